// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_mem_columns_header() -- do not edit
#pragma once
#include <cstdint>
namespace olatgm {
constexpr uint32_t COL_CMP_ABS_DIFF = 3u;
constexpr uint32_t COL_CMP_ABS_DIFF_INV = 4u;
constexpr uint32_t COL_CMP_FILTER_LOOKING_RC = 5u;
constexpr uint32_t COL_CMP_GTE = 2u;
constexpr uint32_t COL_CMP_OP0 = 0u;
constexpr uint32_t COL_CMP_OP1 = 1u;
constexpr uint32_t COL_MEM_ADDR = 3u;
constexpr uint32_t COL_MEM_CLK = 4u;
constexpr uint32_t COL_MEM_DIFF_ADDR = 19u;
constexpr uint32_t COL_MEM_DIFF_ADDR_COND = 22u;
constexpr uint32_t COL_MEM_DIFF_ADDR_INV = 20u;
constexpr uint32_t COL_MEM_DIFF_CLK = 21u;
constexpr uint32_t COL_MEM_ENV_IDX = 1u;
constexpr uint32_t COL_MEM_FILTER_LOOKING_RC = 27u;
constexpr uint32_t COL_MEM_FILTER_LOOKING_RC_COND = 28u;
constexpr uint32_t COL_MEM_IS_RW = 2u;
constexpr uint32_t COL_MEM_IS_WRITE = 17u;
constexpr uint32_t COL_MEM_OP = 5u;
constexpr uint32_t COL_MEM_RC_VALUE = 26u;
constexpr uint32_t COL_MEM_REGION_HEAP = 25u;
constexpr uint32_t COL_MEM_REGION_PROPHET = 24u;
constexpr uint32_t COL_MEM_RW_ADDR_UNCHANGED = 23u;
constexpr uint32_t COL_MEM_S_CALL = 8u;
constexpr uint32_t COL_MEM_S_MLOAD = 6u;
constexpr uint32_t COL_MEM_S_MSTORE = 7u;
constexpr uint32_t COL_MEM_S_POSEIDON = 13u;
constexpr uint32_t COL_MEM_S_PROPHET = 16u;
constexpr uint32_t COL_MEM_S_RET = 9u;
constexpr uint32_t COL_MEM_S_SCCALL = 12u;
constexpr uint32_t COL_MEM_S_SLOAD = 15u;
constexpr uint32_t COL_MEM_S_SSTORE = 14u;
constexpr uint32_t COL_MEM_S_TLOAD = 10u;
constexpr uint32_t COL_MEM_S_TSTORE = 11u;
constexpr uint32_t COL_MEM_TX_IDX = 0u;
constexpr uint32_t COL_MEM_VALUE = 18u;
constexpr uint32_t NUM_MEM_COLS = 29u, COL_NUM_CMP = 6u;
constexpr uint64_t ADDR_HEAP_PTR = 18446744060824649731ull;
constexpr uint64_t MEM_OP_MASK_CALL = 16777216ull; constexpr uint32_t MEM_OP_RANK_CALL = 0u;
constexpr uint64_t MEM_OP_MASK_MLOAD = 4194304ull; constexpr uint32_t MEM_OP_RANK_MLOAD = 1u;
constexpr uint64_t MEM_OP_MASK_MSTORE = 2097152ull; constexpr uint32_t MEM_OP_RANK_MSTORE = 2u;
constexpr uint64_t MEM_OP_MASK_POSEIDON = 4096ull; constexpr uint32_t MEM_OP_RANK_POSEIDON = 3u;
constexpr uint64_t MEM_OP_MASK_RET = 8388608ull; constexpr uint32_t MEM_OP_RANK_RET = 4u;
constexpr uint64_t MEM_OP_MASK_SLOAD = 2048ull; constexpr uint32_t MEM_OP_RANK_SLOAD = 5u;
constexpr uint64_t MEM_OP_MASK_SSTORE = 1024ull; constexpr uint32_t MEM_OP_RANK_SSTORE = 6u;
constexpr uint64_t MEM_OP_MASK_TLOAD = 512ull; constexpr uint32_t MEM_OP_RANK_TLOAD = 7u;
constexpr uint64_t MEM_OP_MASK_TSTORE = 256ull; constexpr uint32_t MEM_OP_RANK_TSTORE = 8u;
constexpr uint32_t MEM_OPS = 9u, MEM_CELL_WORDS = 5u;
}  // namespace olatgm
