// k_circuit_ops.hpp — the device steps the circuit kernels share, each defined once: the recursion circuit's witness
// program (k_witness.hpp), a caller's circuit checked (k_user_circuit.hpp) and evaluated (k_circuit_eval.hpp).  The
// variable accessor and the word helpers, the eleven ops W_CONST .. W_BIT (circuit_op), the gate value, the Poseidon
// invocation.  What a kernel does with a result — compare or store it, which lane owns which witness, what it reports —
// is the kernel's own.
#pragma once
#include "layout.hpp"
#include "poseidon2.hpp"

namespace rsv {

__device__ __forceinline__ QM31 q_of(uint4 v) { return q_mk(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ uint4 u4_of(QM31 q) { return make_uint4(q.a.a, q.a.b, q.b.a, q.b.b); }
__device__ __forceinline__ uint4 u4_words(const uint32_t* w) { return make_uint4(w[0], w[1], w[2], w[3]); }
__device__ __forceinline__ bool uc_canonical(uint4 v) { return v.x < P && v.y < P && v.z < P && v.w < P; }

// vars[n][n_vars] (by_variable = 0) or vars[n_vars][n]
template <class T>
__device__ __forceinline__ T& var_at(T* vars, bool by_variable, size_t n, size_t n_vars, uint32_t p, uint32_t w) {
    return by_variable ? vars[w * n + p] : vars[p * n_vars + w];
}

// An instruction's value (w0 = op, dst, a, b; w1 = imm0..3): the ops W_CONST .. W_BIT here, rd(v) = variable v; any other
// op is the caller's own, other() — the switch's default, so that a kernel still branches once on the op.
template <class Rd, class Other>
__device__ __forceinline__ uint4 circuit_op(const uint4 w0, const uint4 w1, Rd rd, Other other) {
    const uint32_t x = w0.z, y = w0.w, i0 = w1.x;
    uint4 r = make_uint4(0, 0, 0, 0);
    switch (w0.x) {
    case W_CONST: r = w1; break;
    case W_ADD: r = u4_of(q_add(q_of(rd(x)), q_of(rd(y)))); break;
    case W_MUL: r = u4_of(q_mul(q_of(rd(x)), q_of(rd(y)))); break;
    case W_MULC: r = u4_of(q_mul_m(q_of(rd(x)), i0)); break;
    case W_COPY: r = rd(x); break;
    case W_INV: r.x = m_inv(rd(x).x); break;  // 0 -> 0
    case W_INV0: r.x = m_inv(rd(x).x); break;
    case W_QINV: {
        const uint4 v = rd(x);
        if (v.x | v.y | v.z | v.w) r = u4_of(q_inv(q_of(v)));
        break;
    }
    case W_CINV: {
        const uint4 v = rd(x);
        if (v.x | v.y) {
            const CM31 c = c_inv(c_mk(v.x, v.y));
            r.x = i0 ? c.b : c.a;
        }
        break;
    }
    case W_COORD: {
        const uint4 v = rd(x);
        r.x = i0 == 0 ? v.x : i0 == 1 ? v.y : i0 == 2 ? v.z : v.w;
        break;
    }
    case W_BIT: r.x = (rd(x).x >> i0) & 1u; break;
    default: r = other(); break;
    }
    return r;
}

// op (a + b) + (1 - op) a b; at a witness-op row op is `op` where variable `bit` is not zero, else 0
template <class Rd>
__device__ __forceinline__ QM31 gate_value(uint4 va, uint4 vb, uint32_t op, bool witness_op, uint32_t bit, Rd rd) {
    if (witness_op) op = rd(bit).x ? op : 0u;
    const QM31 qa = q_of(va), qb = q_of(vb);
    return q_add(q_mul_m(q_add(qa, qb), op), q_mul_m(q_mul(qa, qb), m_sub(1u, op)));
}

// One invocation: in = r1, r2 as gathered, sw its swap bit, good = what the caller asks beyond canonical input words.  The
// permutation takes canonical words only: where the verdict fails it runs on a zero state.  Writes the record f[0..8) (the
// inputs as given, then the output) and the swap byte, hands output quarter q to out(q, value) as it is stored -> the verdict.
template <class Out>
__device__ __forceinline__ bool poseidon_invoke(const uint4 (&in)[4], uint32_t sw, bool good, uint4* f, uint8_t* swap, Out out) {
    good &= uc_canonical(in[0]) & uc_canonical(in[1]) & uc_canonical(in[2]) & uc_canonical(in[3]);  // no branch: a lane's latency counts
    State16 st;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint4 v = sw ? in[(q + 2) & 3] : in[q];
        if (!good) v = make_uint4(0, 0, 0, 0);
        st.s[4 * q] = v.x; st.s[4 * q + 1] = v.y; st.s[4 * q + 2] = v.z; st.s[4 * q + 3] = v.w;
    }
    st = poseidon2(st);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 o = make_uint4(st.s[4 * q], st.s[4 * q + 1], st.s[4 * q + 2], st.s[4 * q + 3]);
        f[q] = in[q];
        f[4 + q] = o;
        out(q, o);
    }
    *swap = (uint8_t)sw;
    return good;
}

}  // namespace rsv
