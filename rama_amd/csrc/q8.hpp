// q8.hpp -- llama2.c Q8_0 decode kernels (runq.c's quantized products with rama's per-op semantics elsewhere).
//
// Numeric definition:
//   quantize(x, GS), per group of GS consecutive floats: wmax = max |x|; scale = wmax / 127.0f (IEEE division);
//     q = (int8) clamp(C round(x / scale), -127, 127) -- a correctly rounded division, then round half away from zero;
//     scale == 0 gives q = 0.  Denormals are kept.
//   matmul(o, xq, Wq), row i: val = +0.0f; for g = 0, 1, ... IN ORDER: ival = sum_k xq[g GS + k] * Wq[i][g GS + k] (exact
//     int32), val = val + ((float)ival * Ws[i][g]) * xs[g] -- three separately rounded fp32 operations, no contraction.
// Everything else in the forward (norms, RoPE, attention, SiLU, residual adds) is parity mode's exact kernels.
#pragma once
#define RAMA_Q8_HPP 1           // (q8_serve_api.hip and q8_spec_api.hip refuse to be compiled with this header or q8_batch.hpp: their kernels are q8_api.hip's)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ref_order.hpp"

namespace rama {

typedef __attribute__((ext_vector_type(4))) int i4;

constexpr int kQ8Waves = 4;            // waves per workgroup of the Q8 matvec
constexpr int kQ8Unroll = 4;           // 16-byte chunks per lane and row issued before any of them is consumed

enum { Q8EPI_STORE = 0, Q8EPI_RESID = 1, Q8EPI_SWIGLU = 2 };

struct Q8MatParams {
    const int8_t* w[3]; const float* ws[3]; float* o[3];   // up to three matrices [rows, K] with the same activations
    const int8_t* xq; const float* xs;                     // quantized activations [K], scales [K / gs]
    int K, rows, gs, nmat;
};

// ---------------------------------------------------------------- activations: quantize(x, n, GS), one wave per group
__device__ __forceinline__ float q8_wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int8_t q8_round_act(float x, float scale) {
    RAMA_NO_CONTRACT
    if (scale == 0.0f) return 0;
    float r = roundf(x / scale);                   // C round: halves away from zero
    r = fminf(fmaxf(r, -127.0f), 127.0f);
    return (int8_t)(int)r;
}

__global__ __launch_bounds__(256) void q8_quantize_kernel(const float* __restrict__ x, int n, int gs, int8_t* __restrict__ q, float* __restrict__ s) {
    RAMA_NO_CONTRACT
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g * gs >= n) return;
    const float* xg = x + (size_t)g * gs;
    float m = 0.0f;
    for (int i = lane; i < gs; i += 64) m = fmaxf(m, fabsf(xg[i]));
    m = q8_wave_max(m);                            // max is exact in any order
    const float scale = m / 127.0f;
    for (int i = lane; i < gs; i += 64) q[(size_t)g * gs + i] = q8_round_act(xg[i], scale);
    if (lane == 0) s[g] = scale;
}

// ---------------------------------------------------------------- the Q8 matvec
// A wave owns RW rows (Q8EPI_SWIGLU: row i of W1 and of W3).  Lane l streams 16-byte chunks l, l + 64, ... of each row with non-temporal
// loads, kQ8Unroll chunks per row in flight before any is consumed, and takes four v_dot4_i32_i8 per chunk against the same chunk of xq.
// A group is GS / 16 consecutive chunks, i.e. consecutive lanes of one load: their exact int32 sums meet by xor shuffles, and the group's
// first lane forms ((float)ival * ws) * xs into LDS.  The in-order fp32 sum over groups is then one lane per row.
// Needs K % 16 == 0 and GS a power of two in [16, 1024] (q8_matvec_fast_ok); q8_matvec_generic_kernel takes every other shape.
__device__ __forceinline__ int q8_dot16(const i4 a, const i4 b) {
    int d = __builtin_amdgcn_sdot4(a.x, b.x, 0, false);
    d = __builtin_amdgcn_sdot4(a.y, b.y, d, false);
    d = __builtin_amdgcn_sdot4(a.z, b.z, d, false);
    return __builtin_amdgcn_sdot4(a.w, b.w, d, false);
}

template <int RW, int EPI>
__global__ __launch_bounds__(kQ8Waves * 64) void q8_matvec_kernel(Q8MatParams p) {
    RAMA_NO_CONTRACT
    extern __shared__ float s_terms[];                          // [kQ8Waves][RW][G]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int G = p.K / p.gs, cpg = p.gs / 16, nch = p.K / 16;
    float* terms = s_terms + (size_t)wv * RW * G;
    const int task = blockIdx.x * kQ8Waves + wv;
    const int total = EPI == Q8EPI_SWIGLU ? p.rows : p.nmat * p.rows;
    const int8_t* wrow[RW]; const float* srow[RW]; bool ok[RW];
#pragma unroll
    for (int r = 0; r < RW; r++) {
        int m, i;
        if (EPI == Q8EPI_SWIGLU) { m = r; i = task; ok[r] = task < p.rows; }
        else { const int vr = task * RW + r; ok[r] = vr < total; m = ok[r] ? vr / p.rows : 0; i = ok[r] ? vr - m * p.rows : 0; }
        wrow[r] = p.w[m] + (size_t)i * p.K;
        srow[r] = p.ws[m] + (size_t)i * G;
    }
    const i4* x4 = reinterpret_cast<const i4*>(p.xq);
    for (int j0 = 0; j0 * 64 < nch; j0 += kQ8Unroll) {
        i4 wc[kQ8Unroll][RW], xc[kQ8Unroll];
#pragma unroll
        for (int u = 0; u < kQ8Unroll; u++) {
            const int c = (j0 + u) * 64 + lane;
            const bool in = c < nch;
            xc[u] = in ? x4[c] : i4{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < RW; r++)
                wc[u][r] = (in && ok[r]) ? __builtin_nontemporal_load(reinterpret_cast<const i4*>(wrow[r]) + c) : i4{0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < kQ8Unroll; u++) {
            const int c = (j0 + u) * 64 + lane;
            if ((j0 + u) * 64 >= nch) break;                   // wave-uniform
#pragma unroll
            for (int r = 0; r < RW; r++) {
                int d = q8_dot16(wc[u][r], xc[u]);
                for (int off = 1; off < cpg; off <<= 1) d += __shfl_xor(d, off, 64);
                if (c < nch && ok[r] && (lane & (cpg - 1)) == 0) {
                    const int g = c / cpg;
                    terms[r * G + g] = ((float)d * srow[r][g]) * p.xs[g];
                }
            }
        }
    }
    __syncthreads();
    float val = 0.0f;
    if (lane < RW) {
        const float* t = terms + lane * G;
        for (int g = 0; g < G; g++) val = val + t[g];
    }
    if (EPI == Q8EPI_SWIGLU) {
        const float v3 = __shfl(val, 1, 64);
        if (lane == 0 && ok[0]) {
            const float a = val;
            const float sg = a * (1.0f / (1.0f + expf_glibc(-a)));      // cpu.rs:54-57 sinu
            p.o[0][task] = sg * v3;                                     // cpu.rs:59-64 array_mult
        }
        return;
    }
    if (lane < RW) {
        float vsel = val;
        bool oks = false; int m = 0, i = 0;
#pragma unroll
        for (int r = 0; r < RW; r++) if (r == lane) { oks = ok[r]; const int vr = task * RW + r; m = oks ? vr / p.rows : 0; i = oks ? vr - m * p.rows : 0; }
        if (oks) {
            if (EPI == Q8EPI_RESID) p.o[m][i] = p.o[m][i] + vsel;     // infer.rs:37 / :47 (array_add)
            else p.o[m][i] = vsel;
        }
    }
}

// every other shape (any K, any group size dividing it): one thread per row (and matrix), bytewise, the same arithmetic
template <int EPI>
__global__ void q8_matvec_generic_kernel(Q8MatParams p) {
    RAMA_NO_CONTRACT
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = EPI == Q8EPI_SWIGLU ? p.rows : p.nmat * p.rows;
    if (t >= total) return;
    const int G = p.K / p.gs;
    float v[2] = {0.0f, 0.0f};
    const int nm = EPI == Q8EPI_SWIGLU ? 2 : 1;
    int m0 = EPI == Q8EPI_SWIGLU ? 0 : t / p.rows, i = EPI == Q8EPI_SWIGLU ? t : t - (t / p.rows) * p.rows;
    for (int mm = 0; mm < nm; mm++) {
        const int m = m0 + mm;
        const int8_t* wr = p.w[m] + (size_t)i * p.K;
        const float* sr = p.ws[m] + (size_t)i * G;
        float val = 0.0f;
        for (int g = 0; g < G; g++) {
            int d = 0;
            for (int k = 0; k < p.gs; k++) d += (int)p.xq[g * p.gs + k] * (int)wr[g * p.gs + k];
            val = val + ((float)d * sr[g]) * p.xs[g];
        }
        v[mm] = val;
    }
    if (EPI == Q8EPI_SWIGLU) {
        const float a = v[0];
        const float sg = a * (1.0f / (1.0f + expf_glibc(-a)));
        p.o[0][i] = sg * v[1];
    } else if (EPI == Q8EPI_RESID) {
        p.o[m0][i] = p.o[m0][i] + v[0];
    } else {
        p.o[m0][i] = v[0];
    }
}

static inline bool q8_matvec_fast_ok(int K, int gs) {
    return K % 16 == 0 && gs >= 16 && gs <= 1024 && (gs & (gs - 1)) == 0 && K % gs == 0;
}

}  // namespace rama
