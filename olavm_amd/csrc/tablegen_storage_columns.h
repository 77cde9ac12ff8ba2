// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_storage_columns_header() -- do not edit
#pragma once
#include <cstdint>
namespace olatgs {
constexpr uint32_t COL_ST_ACCESS_IDX = 0u;
constexpr uint32_t COL_ST_ACC_LAYER_MARKER = 43u;
constexpr uint32_t COL_ST_ADDR_ACC = 12u;
constexpr uint32_t COL_ST_ADDR_RANGE_START = 13u, COL_ST_ADDR_RANGE_END = 17u;
constexpr uint32_t COL_ST_FILTER_IS_FOR_PROG = 46u;
constexpr uint32_t COL_ST_FILTER_IS_HASH_BIT_0 = 44u;
constexpr uint32_t COL_ST_FILTER_IS_HASH_BIT_1 = 45u;
constexpr uint32_t COL_ST_HASH_RANGE_START = 34u, COL_ST_HASH_RANGE_END = 38u;
constexpr uint32_t COL_ST_HASH_TYPE = 29u;
constexpr uint32_t COL_ST_IS_LAYER_1 = 38u;
constexpr uint32_t COL_ST_IS_LAYER_128 = 40u;
constexpr uint32_t COL_ST_IS_LAYER_192 = 41u;
constexpr uint32_t COL_ST_IS_LAYER_256 = 42u;
constexpr uint32_t COL_ST_IS_LAYER_64 = 39u;
constexpr uint32_t COL_ST_IS_PADDING = 47u;
constexpr uint32_t COL_ST_IS_WRITE = 9u;
constexpr uint32_t COL_ST_LAYER = 10u;
constexpr uint32_t COL_ST_LAYER_BIT = 11u;
constexpr uint32_t COL_ST_PATH_RANGE_START = 21u, COL_ST_PATH_RANGE_END = 25u;
constexpr uint32_t COL_ST_PRE_HASH_RANGE_START = 30u, COL_ST_PRE_HASH_RANGE_END = 34u;
constexpr uint32_t COL_ST_PRE_PATH_RANGE_START = 17u, COL_ST_PRE_PATH_RANGE_END = 21u;
constexpr uint32_t COL_ST_PRE_ROOT_RANGE_START = 1u, COL_ST_PRE_ROOT_RANGE_END = 5u;
constexpr uint32_t COL_ST_ROOT_RANGE_START = 5u, COL_ST_ROOT_RANGE_END = 9u;
constexpr uint32_t COL_ST_SIB_RANGE_START = 25u, COL_ST_SIB_RANGE_END = 29u;
constexpr uint32_t NUM_COL_ST = 48u, NUM_POSEIDON_COLS = 134u;
constexpr uint32_t STORAGE_ACCESS_WORDS = 14u, STORAGE_DEPTH = 256u;
}  // namespace olatgs
