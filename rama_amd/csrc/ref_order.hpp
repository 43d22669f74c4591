// ref_order.hpp -- the decode step in the REFERENCE'S OWN ARITHMETIC ORDER (opt-in:
// rama_set_tuning(ctx, "ref_order", 1)).
//
// The fast path (kernels.hpp) sums every dot product in a tree with fused multiply-adds; the
// reference's CPU backend sums 4 strided lanes sequentially with separate multiplies and adds
// (engine/src/device/cpu.rs:127-153) and carries ~1.4e-4 of rounding error in the llama2-7B logits
// (profiles/r02_parity_llama2_7b_200pos.json: oracle vs the fp64-accumulated network), so no
// implementation that sums differently can stay within 1e-4 of it over a long generation -- being
// closer to the exact result does not help.  This file reproduces the reference's rounding sequence
// operation by operation instead, so that the HIP path can be compared with it BIT FOR BIT:
//   matmul               cpu.rs:127-153   4 lane sums over k = j (mod 4), product and sum rounded
//                                         separately, (l0 + l1) + (l2 + l3)
//   rmsnorm              cpu.rs:99-117    sequential sum of squares, w * (v * x)
//   apply_position       cpu.rs:74-97     a*c - b*s with three roundings
//   multi_head_attention cpu.rs:23-52     sequential q.k per timestep, / sqrt(hs); softmax: max,
//                                         exp, sequential sum, divide; xb += att * v, t ascending
//   sinu / array_mult    cpu.rs:54-64     a * (1 / (1 + exp(-a))), then * hb2
// exp is glibc's expf (what Rust's f32::exp calls on Linux), restated below from the binary of this
// image's libm (2.35, the FMA ifunc variant every AVX2 host selects): table-driven, evaluated in
// double, with the same four fused multiply-adds.  Everything here is parallel only across
// independent outputs (rows, timesteps, head columns); every sum that the reference orders is one
// thread's sequential loop.  Speed is not the point (~8 ms per llama2-7B token).
#pragma once
#include "kernels.hpp"

namespace rama {

// every function below must round a*b + c twice: hipcc contracts by default
#define RAMA_NO_CONTRACT _Pragma("clang fp contract(off)")

// ---------------------------------------------------------------- glibc 2.35 expf, FMA variant
// sysdeps/ieee754/flt-32/e_expf.c + e_exp2f_data.c (N = 32), as compiled with -mfma:
//   kd = fma(InvLn2N, x, Shift); ki = bits(kd); kd -= Shift; r = fma(InvLn2N, x, -kd)
//   s = double(T[ki % 32] + (ki << 47)); z = fma(C0, r, C1); y = fma(C2, r, 1); y = fma(z, r*r, y)
//   return float(y * s)
__device__ __constant__ const unsigned long long kExp2fTab[32] = {
    0x3ff0000000000000ULL, 0x3fefd9b0d3158574ULL, 0x3fefb5586cf9890fULL, 0x3fef9301d0125b51ULL,
    0x3fef72b83c7d517bULL, 0x3fef54873168b9aaULL, 0x3fef387a6e756238ULL, 0x3fef1e9df51fdee1ULL,
    0x3fef06fe0a31b715ULL, 0x3feef1a7373aa9cbULL, 0x3feedea64c123422ULL, 0x3feece086061892dULL,
    0x3feebfdad5362a27ULL, 0x3feeb42b569d4f82ULL, 0x3feeab07dd485429ULL, 0x3feea47eb03a5585ULL,
    0x3feea09e667f3bcdULL, 0x3fee9f75e8ec5f74ULL, 0x3feea11473eb0187ULL, 0x3feea589994cce13ULL,
    0x3feeace5422aa0dbULL, 0x3feeb737b0cdc5e5ULL, 0x3feec49182a3f090ULL, 0x3feed503b23e255dULL,
    0x3feee89f995ad3adULL, 0x3feeff76f2fb5e47ULL, 0x3fef199bdd85529cULL, 0x3fef3720dcef9069ULL,
    0x3fef5818dcfba487ULL, 0x3fef7c97337b9b5fULL, 0x3fefa4afa2a490daULL, 0x3fefd0765b6e4540ULL,
};

// tab: the 32 table words -- kExp2fTab itself, or a workgroup's copy of it in LDS (exp_tab_fill).  A lookup in constant memory is a per-lane load
// that travels to L2 (and past it once a long context's cache rows have pushed the table out): ~0.2 us in front of EVERY exponential of a loop,
// 1.5 of the 19 us of the long-context softmax + values launch at position 1 900 ([r5]: an LDS read instead).
__device__ __forceinline__ float expf_glibc_tab(float x, const unsigned long long* tab) {
    const unsigned ux = __float_as_uint(x);
    const unsigned abstop = (ux >> 20) & 0x7ff;
    if (abstop > 0x42a) {                                   // |x| >= 88 or not finite
        if (ux == 0xff800000u) return 0.0f;                 // exp(-inf)
        if (abstop > 0x7f7) return x + x;                   // inf, nan
        if (x > 0x1.62e42ep6f) return __uint_as_float(0x7f800000u);     // overflow
        if (x < -0x1.9fe368p6f) return 0.0f;                // underflow
    }
    const double xd = (double)x;
    const double InvLn2N = 0x1.71547652b82fep+0 * 32.0, Shift = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0, C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0, C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
    double kd = __builtin_fma(InvLn2N, xd, Shift);
    const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
    kd = __dsub_rn(kd, Shift);
    const double r = __builtin_fma(InvLn2N, xd, -kd);
    const unsigned long long t = tab[ki & 31] + (ki << 47);
    const double s = __longlong_as_double((long long)t);
    const double z = __builtin_fma(C0, r, C1);
    const double r2 = __dmul_rn(r, r);
    double y = __builtin_fma(C2, r, 1.0);
    y = __builtin_fma(z, r2, y);
    y = __dmul_rn(y, s);
    return (float)y;
}
__device__ __forceinline__ float expf_glibc(float x) { return expf_glibc_tab(x, kExp2fTab); }
// the table into LDS: threads 0..31 of the workgroup write it; a barrier of the caller's stands between this and the first expf_glibc_tab
__device__ __forceinline__ void exp_tab_fill(unsigned long long* s_tab) { if (threadIdx.x < 32) s_tab[threadIdx.x] = kExp2fTab[threadIdx.x]; }

// ---------------------------------------------------------------- cpu.rs:127-153 matmul, o_cols == 1 (matvec_ref_kernel, ref_kernels.hpp)
// One thread per output row: v_j += a[r][4i + j] * b[4i + j] for i ascending, four chains, then
// (v0 + v1) + (v2 + v3).  Up to 3 matrices per launch (blockIdx.y), all [rows, K].
// lane_reduce: the order of the final sum of the four chains, cpu.rs:148 `v.reduce_add()` -- wide::f32x4 leaves it to the build's target features (an SSE3
// hadd pair, the SSE2 movehl + shuffle idiom, or an array sum), the oracle has the same switch (oracle_set_lane_reduce), "lane_reduce" sets it
enum { LANES_PAIRWISE = 0, LANES_STRIDED = 1, LANES_SEQUENTIAL = 2 };
struct RefMatParams { const float* w[3]; float* o[3]; const float* x; int K, rows; int lane_reduce; };

// ---------------------------------------------------------------- cpu.rs:74-97 apply_position, all heads

// cpu.rs:74-97 apply_position over all heads + the two cache appends of infer.rs:31-33, the position taken from the device cursor: table row pos,
// cache row pos (rope_ref_kernel, with the position given: ref_kernels.hpp).  Shared with q8_api.hip (rama_q8_forward's launch), hence `inline`: see kernels.hpp "small ops"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"      // ("another compiler ignores `inline` on a kernel": this one does not)
inline __global__ void rope_ref_cursor_kernel(float* q, float* k, const float* v, const float* fr, const float* fi, int dim, int head_size,
                                       float* kc, float* vc, const Ctl* ctl) {
    RAMA_NO_CONTRACT
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dim / 2) return;
    const int pos = ctl->pos;
    const int i = j % (head_size / 2);
    const float fcr = fr[(size_t)pos * (head_size / 2) + i], fci = fi[(size_t)pos * (head_size / 2) + i];
    const float q0 = q[2 * j], q1 = q[2 * j + 1];
    const float a0 = q0 * fcr - q1 * fci, a1 = q0 * fci + q1 * fcr;
    q[2 * j] = a0; q[2 * j + 1] = a1;
    const float k0 = k[2 * j], k1 = k[2 * j + 1];
    const float b0 = k0 * fcr - k1 * fci, b1 = k0 * fci + k1 * fcr;
    k[2 * j] = b0; k[2 * j + 1] = b1;
    kc[(size_t)pos * dim + 2 * j] = b0; kc[(size_t)pos * dim + 2 * j + 1] = b1;           // infer.rs:32
    vc[(size_t)pos * dim + 2 * j] = v[2 * j]; vc[(size_t)pos * dim + 2 * j + 1] = v[2 * j + 1];   // infer.rs:33
}

// ---------------------------------------------------------------- cpu.rs:23-52 multi_head_attention (attention_ref_kernel, ref_kernels.hpp)
// One workgroup per head; att scratch in LDS (pos + 1 floats) and, when `att` is given, in the
// reference's att[h * seq_len + t] buffer too.
struct RefAttnParams {
    const float* q; const float* kc; const float* vc;     // kc / vc: this layer's slabs [seq, dim]
    float* att; float* xb;
    const Ctl* ctl; int pos_val;
    int dim, head_size, seq_len;
    float* sc = nullptr;      // spread attention (chain.hpp): where the scores launch leaves the raw scores ([n_heads, seq_len]; == att for the three-launch form)
    // a grid of (heads, tokens) -- the parity-mode prefill pass, chain.hpp: token y sits at position pos + y, its q / xb
    // rows are y * tok_stride floats further on, its att rows y * att_stride.  (0, 0 and gridDim.y = 1: one token.)
    int tok_stride, att_stride;
    // ... or tokens of independent sequences (rama_decode_batch in parity mode): token y reads its position and its cache
    // bases from seqs[y] (+ layer_off floats for this layer); pos / kc / vc above are then unused
    const SeqSlot* seqs; size_t layer_off;
};

}  // namespace rama
