// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_columns_header() -- do not edit
#pragma once
#include <cstdint>
namespace olatg {
constexpr uint32_t BW_COMPRESS_LIMBS_START = 29u, BW_COMPRESS_LIMBS_END = 33u;
constexpr uint32_t BW_COMPRESS_PERMUTED_START = 33u, BW_COMPRESS_PERMUTED_END = 37u;
constexpr uint32_t BW_FILTER = 0u;
constexpr uint32_t BW_FIX_BITWSIE_OP0 = 51u;
constexpr uint32_t BW_FIX_BITWSIE_OP1 = 52u;
constexpr uint32_t BW_FIX_BITWSIE_RES = 53u;
constexpr uint32_t BW_FIX_COMPRESS = 54u;
constexpr uint32_t BW_FIX_COMPRESS_PERMUTED_START = 55u, BW_FIX_COMPRESS_PERMUTED_END = 59u;
constexpr uint32_t BW_FIX_RANGE_CHECK_U8 = 37u;
constexpr uint32_t BW_FIX_RANGE_CHECK_U8_PERMUTED_START = 38u, BW_FIX_RANGE_CHECK_U8_PERMUTED_END = 50u;
constexpr uint32_t BW_FIX_TAG = 50u;
constexpr uint32_t BW_OP0 = 2u;
constexpr uint32_t BW_OP0_LIMBS_START = 5u, BW_OP0_LIMBS_END = 9u;
constexpr uint32_t BW_OP0_LIMBS_PERMUTED_START = 17u, BW_OP0_LIMBS_PERMUTED_END = 21u;
constexpr uint32_t BW_OP1 = 3u;
constexpr uint32_t BW_OP1_LIMBS_START = 9u, BW_OP1_LIMBS_END = 13u;
constexpr uint32_t BW_OP1_LIMBS_PERMUTED_START = 21u, BW_OP1_LIMBS_PERMUTED_END = 25u;
constexpr uint32_t BW_RES = 4u;
constexpr uint32_t BW_RES_LIMBS_START = 13u, BW_RES_LIMBS_END = 17u;
constexpr uint32_t BW_RES_LIMBS_PERMUTED_START = 25u, BW_RES_LIMBS_PERMUTED_END = 29u;
constexpr uint32_t BW_TAG = 1u;
constexpr uint32_t COL_NUM_BITWISE = 59u;
constexpr uint32_t COL_NUM_RC = 12u;
constexpr uint32_t COL_PROG_CODE_ADDR_RANGE_START = 0u, COL_PROG_CODE_ADDR_RANGE_END = 4u;
constexpr uint32_t COL_PROG_COMP_PROG = 6u;
constexpr uint32_t COL_PROG_COMP_PROG_PERM = 7u;
constexpr uint32_t COL_PROG_EXEC_CODE_ADDR_RANGE_START = 8u, COL_PROG_EXEC_CODE_ADDR_RANGE_END = 12u;
constexpr uint32_t COL_PROG_EXEC_COMP_PROG = 14u;
constexpr uint32_t COL_PROG_EXEC_COMP_PROG_PERM = 15u;
constexpr uint32_t COL_PROG_EXEC_INST = 13u;
constexpr uint32_t COL_PROG_EXEC_PC = 12u;
constexpr uint32_t COL_PROG_FILTER_EXEC = 16u;
constexpr uint32_t COL_PROG_FILTER_PROG_CHUNK = 17u;
constexpr uint32_t COL_PROG_INST = 5u;
constexpr uint32_t COL_PROG_PC = 4u;
constexpr uint32_t NUM_PROG_COLS = 18u;
constexpr uint32_t RC_CMP_FILTER = 3u;
constexpr uint32_t RC_CPU_FILTER = 0u;
constexpr uint32_t RC_FIX_RANGE_CHECK_U16 = 9u;
constexpr uint32_t RC_FIX_RANGE_CHECK_U16_PERMUTED_HI = 11u;
constexpr uint32_t RC_FIX_RANGE_CHECK_U16_PERMUTED_LO = 10u;
constexpr uint32_t RC_LIMB_HI = 6u;
constexpr uint32_t RC_LIMB_HI_PERMUTED = 8u;
constexpr uint32_t RC_LIMB_LO = 5u;
constexpr uint32_t RC_LIMB_LO_PERMUTED = 7u;
constexpr uint32_t RC_MEMORY_REGION_FILTER = 2u;
constexpr uint32_t RC_MEMORY_SORT_FILTER = 1u;
constexpr uint32_t RC_VAL = 4u;
constexpr uint64_t OP_MASK_AND = 262144ull;
constexpr uint64_t OP_MASK_OR = 131072ull;
constexpr uint64_t OP_MASK_XOR = 65536ull;
}  // namespace olatg
