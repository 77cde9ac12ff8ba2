// The constraint program of a table, interpreted on the device: the loop quotient_kernel (stark.hip, on the LDE domain) and
// check_constraints_kernel (check.hip, on the trace domain) share.  It owns the op decode (air_op), the opcodes' meaning and the
// register writes; the program has passed validate_airset (airset_host.h): every register, column and parameter it names exists.
#pragma once
#include "airset_host.h"

namespace ola {

#define QW 64  // one wavefront per workgroup; register file = n_regs x 64 lanes in LDS: register r of lane l at regs[r * QW + l]

// ops: 2 words per op.  load(column, is_next) -> the canonical cell of this lane's row or of the row after it; emit(kind, value).
template <class Load, class Emit>
__device__ __forceinline__ void air_interpret(const u64* __restrict__ ops, u32 n_ops, const u64* __restrict__ params, u64* regs, int lane,
                                              Load load, Emit emit) {
    for (u32 k = 0; k < n_ops; k++) {
        const AirOp o = air_op(ops[2 * k], ops[2 * k + 1]);
        u64 v;
        switch (o.op) {
            case AOP_LOCAL: v = load(o.a, false); break;
            case AOP_NEXT: v = load(o.a, true); break;
            case AOP_CONST: v = o.imm; break;
            case AOP_PARAM: v = params[o.a]; break;
            case AOP_ADD: v = gl_add(regs[o.a * QW + lane], regs[o.b * QW + lane]); break;
            case AOP_SUB: v = gl_sub(regs[o.a * QW + lane], regs[o.b * QW + lane]); break;
            case AOP_MUL: v = gl_mul(regs[o.a * QW + lane], regs[o.b * QW + lane]); break;
            case AOP_ISZERO: v = (regs[o.a * QW + lane] == 0) ? 1 : 0; break;
            default: emit(o.kind, regs[o.a * QW + lane]); continue;
        }
        regs[o.dst * QW + lane] = v;
    }
}

}  // namespace ola
