// q8_batch.hpp -- the Q8_0 product over a batch of tokens (rama_q8_matmul_batch, rama_q8_prefill, rama_q8_decode_batch).
//
// O[t][i] = matmul(xq[t], W)[i] for up to kQ8bMaxTok token rows per launch, with q8.hpp's arithmetic row by row and token by
// token: exact int32 group sums, then val = +0.0f; val = val + ((float)ival * Ws[i][g]) * xs[t][g] for g in order, three
// separately rounded fp32 operations.
//
// The matrix-core kernel: one wave owns a 16-row tile of one matrix (Q8EPI_SWIGLU: the same 16 rows of W1 and of W3) and
// every token of the launch, NT tiles of 16 tokens, so each weight byte and scale is fetched once per launch.
// v_mfma_i32_16x16x64_i8 takes 64 bytes of K for 16 rows x 16 tokens.  Lane l loads the 16 bytes at k offset 16 (l >> 4)
// of row l & 15 (A) and of token l & 15 (B): A and B share one lane -> k map, so the int32 sum is the exact dot product of
// those 64 bytes whatever order the hardware walks k in.
//   GS a multiple of 64: a group is GS / 64 chained MFMAs from a zero accumulator (exact in int32).
//   GS = 32: a 64-byte chunk holds groups 2c (lanes 0..31's bytes) and 2c + 1 (lanes 32..63's); each group is one MFMA
//   with the other group's activation bytes zeroed.  (The last chunk of K = 32 mod 64 holds one group.)
// C/D: lane l holds token l & 15 and rows 4 (l >> 4) + j in register j, so the in-order fp32 sum over groups is per
// accumulator element in registers.  Every other shape goes to q8_gemm_generic_kernel (one thread per row and token).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "q8.hpp"
#include "q8_tree_tables.hpp"      // TreeAnc (q8_rope_tree_node_kernel)

namespace rama {

constexpr int kQ8bWaves = 1;       // waves (row tiles) per workgroup: one, so that the few row tiles of Wo / W2 spread over every CU
// (kQ8bMaxTok, the token rows per launch -- 8 tiles of 16 --, is q8_host.hpp's: the launcher's constant, which the other Q8 translation units check against)

struct Q8BatchParams {
    const int8_t* w[3]; const float* ws[3]; float* o[3];   // up to three matrices [rows, K] over the same activations
    const int8_t* xq; const float* xs;                     // activations [n_tok, K], scales [n_tok, K / gs]
    int K, rows, gs, nmat, n_tok;
    int ostride;                                           // floats from one token's output row to the next
};

__device__ __forceinline__ void q8b_epi_store(const Q8BatchParams& p, int EPI, int m, int row, int t, float v) {
    float* o = p.o[m] + (size_t)t * p.ostride + row;
    if (EPI == Q8EPI_RESID) *o = *o + v;                   // infer.rs:37 / :47 (array_add)
    else *o = v;
}

template <int NT, int EPI, bool G32>
__global__ __launch_bounds__(kQ8bWaves * 64) void q8_gemm_mfma_kernel(Q8BatchParams p) {
    RAMA_NO_CONTRACT
    constexpr int RT = EPI == Q8EPI_SWIGLU ? 2 : 1;
    const int lane = threadIdx.x & 63, qk = lane >> 4, r16 = lane & 15;
    const int tiles = (p.rows + 15) / 16;
    const int task = blockIdx.x * kQ8bWaves + (threadIdx.x >> 6);
    const int total = EPI == Q8EPI_SWIGLU ? tiles : p.nmat * tiles;
    if (task >= total) return;                              // (wave-uniform)
    const int m0 = EPI == Q8EPI_SWIGLU ? 0 : task / tiles;
    const int tile = EPI == Q8EPI_SWIGLU ? task : task - m0 * tiles;
    const int K = p.K, G = K / p.gs, nch = (K + 63) / 64;
    const int arow = tile * 16 + r16;                       // the row this lane loads
    const bool arow_ok = arow < p.rows;
    const int8_t* wa[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) wa[rt] = p.w[m0 + rt] + (size_t)(arow_ok ? arow : 0) * K + qk * 16;
    int crow[4]; bool crow_ok[4];                           // the rows this lane's accumulator registers hold
#pragma unroll
    for (int j = 0; j < 4; j++) { crow[j] = tile * 16 + qk * 4 + j; crow_ok[j] = crow[j] < p.rows; }
    const int8_t* xb[NT]; bool tok_ok[NT];
#pragma unroll
    for (int tb = 0; tb < NT; tb++) {
        const int t = tb * 16 + r16;
        tok_ok[tb] = t < p.n_tok;
        xb[tb] = p.xq + (size_t)(tok_ok[tb] ? t : 0) * K + qk * 16;
    }
    float val[RT][NT][4];
    i4 acc[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int tb = 0; tb < NT; tb++) {
            acc[rt][tb] = i4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; j++) val[rt][tb][j] = 0.0f;
        }
    // the group's term for every accumulator element, added in group order
    auto epilogue = [&](const float (&sc)[RT][4], const float (&xsc)[NT]) {
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int tb = 0; tb < NT; tb++) {
                val[rt][tb][0] = val[rt][tb][0] + ((float)acc[rt][tb].x * sc[rt][0]) * xsc[tb];
                val[rt][tb][1] = val[rt][tb][1] + ((float)acc[rt][tb].y * sc[rt][1]) * xsc[tb];
                val[rt][tb][2] = val[rt][tb][2] + ((float)acc[rt][tb].z * sc[rt][2]) * xsc[tb];
                val[rt][tb][3] = val[rt][tb][3] + ((float)acc[rt][tb].w * sc[rt][3]) * xsc[tb];
                acc[rt][tb] = i4{0, 0, 0, 0};
            }
    };
    const int cpg = G32 ? 1 : p.gs / 64;                    // chunks per group (GS >= 64)
    // a block of U chunks: every load of the block (weights, activations, the scales of the groups it ends) is issued before
    // the first product, so one memory latency is paid per block rather than two per chunk
    constexpr int GPC = G32 ? 2 : 1;                        // groups per chunk
    constexpr int U = (NT <= 1 ? 16 : NT <= 2 ? 8 : NT <= 4 ? 4 : 2) / GPC;
    for (int c0 = 0; c0 < nch; c0 += U) {
        i4 a[U][RT], b[U][NT];
        float sc[U][GPC][RT][4], xsc[U][GPC][NT];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int c = c0 + u, off = c * 64;
            const bool kin = c < nch && off + qk * 16 < K;  // (the second half of the last chunk of K = 32 mod 64 is past the row)
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
                a[u][rt] = (kin && arow_ok) ? __builtin_nontemporal_load(reinterpret_cast<const i4*>(wa[rt] + off)) : i4{0, 0, 0, 0};
#pragma unroll
            for (int tb = 0; tb < NT; tb++) b[u][tb] = (kin && tok_ok[tb]) ? *reinterpret_cast<const i4*>(xb[tb] + off) : i4{0, 0, 0, 0};
#pragma unroll
            for (int h = 0; h < GPC; h++) {
                const int g = G32 ? 2 * c + h : c / cpg;
                const bool gok = c < nch && g < G;
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int j = 0; j < 4; j++) sc[u][h][rt][j] = (gok && crow_ok[j]) ? p.ws[m0 + rt][(size_t)crow[j] * G + g] : 0.0f;
#pragma unroll
                for (int tb = 0; tb < NT; tb++) xsc[u][h][tb] = (gok && tok_ok[tb]) ? p.xs[(size_t)(tb * 16 + r16) * G + g] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int c = c0 + u;
            if (c >= nch) break;                            // wave-uniform
            if (G32) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    if (2 * c + h >= G) break;              // wave-uniform
                    const bool mine = (qk >> 1) == h;       // lanes holding group 2c + h's bytes
#pragma unroll
                    for (int rt = 0; rt < RT; rt++)
#pragma unroll
                        for (int tb = 0; tb < NT; tb++)
                            acc[rt][tb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[u][rt], mine ? b[u][tb] : i4{0, 0, 0, 0}, acc[rt][tb], 0, 0, 0);
                    epilogue(sc[u][h], xsc[u][h]);
                }
            } else {
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int tb = 0; tb < NT; tb++) acc[rt][tb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[u][rt], b[u][tb], acc[rt][tb], 0, 0, 0);
                if ((c + 1) % cpg == 0) epilogue(sc[u][0], xsc[u][0]);
            }
        }
    }
#pragma unroll
    for (int tb = 0; tb < NT; tb++) {
        if (!tok_ok[tb]) continue;
        const int t = tb * 16 + r16;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!crow_ok[j]) continue;
            if (EPI == Q8EPI_SWIGLU) {
                const float a = val[0][tb][j];
                const float sg = a * (1.0f / (1.0f + expf_glibc(-a)));      // cpu.rs:54-57 sinu
                p.o[0][(size_t)t * p.ostride + crow[j]] = sg * val[1][tb][j];  // cpu.rs:59-64 array_mult
            } else {
                q8b_epi_store(p, EPI, m0, crow[j], t, val[0][tb][j]);
            }
        }
    }
}

// The few-token case (up to 32 tokens, GS 32 or 64): K split over the kQ8sWaves waves of one workgroup per row tile, in
// rounds.  In a round wave w takes U consecutive 64-byte chunks (chunk r0 + w U + u) and forms every group term it ends,
// ((float)ival * ws) * xs, into LDS slot (group - first group of the round); after a barrier the workgroup's threads add
// the round's slots in group order onto the values they own (accumulator element e of the tile: e = tid + k 64 kQ8sWaves),
// so the sum over groups is still one in-order chain from +0.0 per (row, token) -- the q8_matvec_kernel idea, bounded by a
// round.  A tile then has kQ8sWaves x U x RT KiB of weights in flight instead of one wave's share.
constexpr int kQ8sWaves = 4;

__host__ __device__ constexpr int q8s_unroll(int NT, int RT, bool G32) { return (16 / (NT * RT)) / (G32 ? 2 : 1); }
__host__ __device__ constexpr size_t q8s_lds_bytes(int NT, int RT, bool G32) {
    return (size_t)kQ8sWaves * q8s_unroll(NT, RT, G32) * (G32 ? 2 : 1) * RT * NT * 256 * sizeof(float);   // <= 64 KiB
}

template <int NT, int EPI, bool G32>
__global__ __launch_bounds__(kQ8sWaves * 64) void q8_gemm_ksplit_kernel(Q8BatchParams p) {
    RAMA_NO_CONTRACT
    constexpr int RT = EPI == Q8EPI_SWIGLU ? 2 : 1;
    constexpr int GPC = G32 ? 2 : 1;
    constexpr int U = q8s_unroll(NT, RT, G32);
    constexpr int S = kQ8sWaves * U * GPC;                  // group slots per round
    constexpr int E = RT * NT * 256;                        // accumulator elements of the tile: ((rt NT + tb) 4 + j) 64 + lane
    constexpr int NTH = kQ8sWaves * 64;
    constexpr int FOLD = (E + NTH - 1) / NTH;               // elements per thread
    static_assert(RT == 1 || (NT * 256) % NTH == 0, "W1 and W3 of one (row, token) must land in one thread");
    extern __shared__ __attribute__((aligned(16))) float s_terms[];   // [S][E]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, qk = lane >> 4, r16 = lane & 15;
    const int tiles = (p.rows + 15) / 16, task = blockIdx.x;
    const int m0 = EPI == Q8EPI_SWIGLU ? 0 : task / tiles;
    const int tile = EPI == Q8EPI_SWIGLU ? task : task - m0 * tiles;
    const int K = p.K, G = K / p.gs, nch = (K + 63) / 64;
    const int arow = tile * 16 + r16;
    const bool arow_ok = arow < p.rows;
    const int8_t* wa[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) wa[rt] = p.w[m0 + rt] + (size_t)(arow_ok ? arow : 0) * K + qk * 16;
    int crow[4]; bool crow_ok[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { crow[j] = tile * 16 + qk * 4 + j; crow_ok[j] = crow[j] < p.rows; }
    const int8_t* xb[NT]; bool tok_ok[NT];
#pragma unroll
    for (int tb = 0; tb < NT; tb++) {
        const int t = tb * 16 + r16;
        tok_ok[tb] = t < p.n_tok;
        xb[tb] = p.xq + (size_t)(tok_ok[tb] ? t : 0) * K + qk * 16;
    }
    float fv[FOLD];
#pragma unroll
    for (int k = 0; k < FOLD; k++) fv[k] = 0.0f;
    for (int r0 = 0; r0 < nch; r0 += kQ8sWaves * U) {
        const int cw = r0 + wave * U;                       // this wave's first chunk of the round
        i4 a[U][RT], b[U][NT];
        float sc[U][GPC][RT][4], xsc[U][GPC][NT];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int c = cw + u, off = c * 64;
            const bool kin = c < nch && off + qk * 16 < K;
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
                a[u][rt] = (kin && arow_ok) ? __builtin_nontemporal_load(reinterpret_cast<const i4*>(wa[rt] + off)) : i4{0, 0, 0, 0};
#pragma unroll
            for (int tb = 0; tb < NT; tb++) b[u][tb] = (kin && tok_ok[tb]) ? *reinterpret_cast<const i4*>(xb[tb] + off) : i4{0, 0, 0, 0};
#pragma unroll
            for (int h = 0; h < GPC; h++) {
                const int g = G32 ? 2 * c + h : c;
                const bool gok = c < nch && g < G;
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int j = 0; j < 4; j++) sc[u][h][rt][j] = (gok && crow_ok[j]) ? p.ws[m0 + rt][(size_t)crow[j] * G + g] : 0.0f;
#pragma unroll
                for (int tb = 0; tb < NT; tb++) xsc[u][h][tb] = (gok && tok_ok[tb]) ? p.xs[(size_t)(tb * 16 + r16) * G + g] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int c = cw + u;
            if (c >= nch) break;                            // wave-uniform
#pragma unroll
            for (int h = 0; h < GPC; h++) {
                if (GPC * c + h >= G) break;                // wave-uniform
                const bool mine = !G32 || (qk >> 1) == h;   // GS 32: lanes holding group 2c + h's bytes
                float* slot = s_terms + (size_t)((wave * U + u) * GPC + h) * E;
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int tb = 0; tb < NT; tb++) {
                        const i4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[u][rt], mine ? b[u][tb] : i4{0, 0, 0, 0}, i4{0, 0, 0, 0}, 0, 0, 0);
                        float* o = slot + (rt * NT + tb) * 256 + lane;
                        o[0] = ((float)d.x * sc[u][h][rt][0]) * xsc[u][h][tb];
                        o[64] = ((float)d.y * sc[u][h][rt][1]) * xsc[u][h][tb];
                        o[128] = ((float)d.z * sc[u][h][rt][2]) * xsc[u][h][tb];
                        o[192] = ((float)d.w * sc[u][h][rt][3]) * xsc[u][h][tb];
                    }
            }
        }
        __syncthreads();
        const int ng = min(S, G - r0 * GPC);                // the round's groups, in order
        for (int sl = 0; sl < ng; sl++)
#pragma unroll
            for (int k = 0; k < FOLD; k++) {
                const int e = tid + k * NTH;
                if (e < E) fv[k] = fv[k] + s_terms[(size_t)sl * E + e];
            }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < FOLD; k++) {
        const int e = tid + k * NTH;
        if (e >= E) continue;
        const int ln = e & 63, j = (e >> 6) & 3, rt = (e >> 8) / NT, tb = (e >> 8) - rt * NT;
        const int row = tile * 16 + (ln >> 4) * 4 + j, t = tb * 16 + (ln & 15);
        if (row >= p.rows || t >= p.n_tok) continue;
        if (EPI == Q8EPI_SWIGLU) {
            if (rt) continue;
            const float a = fv[k], v3 = fv[k + NT * 256 / NTH];                // the same (row, token) of W3
            const float sg = a * (1.0f / (1.0f + expf_glibc(-a)));            // cpu.rs:54-57 sinu
            p.o[0][(size_t)t * p.ostride + row] = sg * v3;                      // cpu.rs:59-64 array_mult
        } else {
            q8b_epi_store(p, EPI, m0, row, t, fv[k]);
        }
    }
}

// every other shape (any K, any group size dividing it, unaligned buffers): one thread per (row [and matrix], token), bytewise
template <int EPI>
__global__ void q8_gemm_generic_kernel(Q8BatchParams p) {
    RAMA_NO_CONTRACT
    const int r = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    const int total = EPI == Q8EPI_SWIGLU ? p.rows : p.nmat * p.rows;
    if (r >= total || t >= p.n_tok) return;
    const int G = p.K / p.gs;
    const int8_t* xq = p.xq + (size_t)t * p.K;
    const float* xs = p.xs + (size_t)t * G;
    const int nm = EPI == Q8EPI_SWIGLU ? 2 : 1;
    const int m0 = EPI == Q8EPI_SWIGLU ? 0 : r / p.rows, i = EPI == Q8EPI_SWIGLU ? r : r - (r / p.rows) * p.rows;
    float v[2] = {0.0f, 0.0f};
    for (int mm = 0; mm < nm; mm++) {
        const int8_t* wr = p.w[m0 + mm] + (size_t)i * p.K;
        const float* sr = p.ws[m0 + mm] + (size_t)i * G;
        float val = 0.0f;
        for (int g = 0; g < G; g++) {
            int d = 0;
            for (int k = 0; k < p.gs; k++) d += (int)xq[g * p.gs + k] * (int)wr[g * p.gs + k];
            val = val + ((float)d * sr[g]) * xs[g];
        }
        v[mm] = val;
    }
    if (EPI == Q8EPI_SWIGLU) {
        const float a = v[0];
        const float sg = a * (1.0f / (1.0f + expf_glibc(-a)));
        p.o[0][(size_t)t * p.ostride + i] = sg * v[1];
    } else {
        q8b_epi_store(p, EPI, m0, i, t, v[0]);
    }
}

static inline bool q8_gemm_mfma_ok(int K, int gs) {
    return K % 16 == 0 && K % gs == 0 && (gs == 32 || (gs % 64 == 0 && gs <= 4096));
}

// infer.rs:25-33 for a token batch: rope_ref_cursor_kernel's arithmetic over a (pairs, tokens) grid.  Token t sits at
// position p0 + t with its cache rows in kc / vc, or -- seqs != NULL -- at seqs[t].pos with its caches at seqs[t].kc / .vc
// + layer_off (a negative position: the row is idle).  Q, Kr, V: [n_tok, dim]; the rotated k goes to Kr and the cache, v to the cache.
__global__ void q8_rope_batch_kernel(float* Q, float* Kr, const float* V, const float* fr, const float* fi, int dim, int head_size,
                                     float* kc, float* vc, int p0, const SeqSlot* seqs, size_t layer_off) {
    RAMA_NO_CONTRACT
    const int j = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (j >= dim / 2) return;
    int pos;
    float *kcb, *vcb;
    if (seqs) {
        pos = seqs[t].pos;
        if (pos < 0) return;               // an idle row of the serving chain's step (q8_serve.hpp): nothing rotated, no cache row
        kcb = seqs[t].kc + layer_off; vcb = seqs[t].vc + layer_off;
    } else { pos = p0 + t; kcb = kc; vcb = vc; }
    float* q = Q + (size_t)t * dim;
    float* k = Kr + (size_t)t * dim;
    const float* v = V + (size_t)t * dim;
    const int i = j % (head_size / 2);
    const float fcr = fr[(size_t)pos * (head_size / 2) + i], fci = fi[(size_t)pos * (head_size / 2) + i];
    const float q0 = q[2 * j], q1 = q[2 * j + 1];
    const float a0 = q0 * fcr - q1 * fci, a1 = q0 * fci + q1 * fcr;
    q[2 * j] = a0; q[2 * j + 1] = a1;
    const float k0 = k[2 * j], k1 = k[2 * j + 1];
    const float b0 = k0 * fcr - k1 * fci, b1 = k0 * fci + k1 * fcr;
    k[2 * j] = b0; k[2 * j + 1] = b1;
    kcb[(size_t)pos * dim + 2 * j] = b0; kcb[(size_t)pos * dim + 2 * j + 1] = b1;           // infer.rs:32
    vcb[(size_t)pos * dim + 2 * j] = v[2 * j]; vcb[(size_t)pos * dim + 2 * j + 1] = v[2 * j + 1];   // infer.rs:33
}

// infer.rs:25-33 for the rows of a tree (q8_tree.hpp): q8_rope_batch_kernel's arithmetic.  The root (row 0) writes its cache row; every
// other live row writes its rotated k and its v into the tree store instead (two rows of one depth share a position).  Kr / V keep the layer's rows.
__global__ void q8_rope_tree_kernel(float* Q, float* Kr, const float* V, const float* fr, const float* fi, int dim, int head_size,
                                    const SeqSlot* seqs, size_t layer_off, float* ks, float* vs) {
    RAMA_NO_CONTRACT
    const int j = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (j >= dim / 2) return;
    const int pos = seqs[t].pos;
    if (pos < 0) return;                   // an idle row: nothing rotated, nothing stored
    // (row 0 is never idle when any row is live; its bases are the sequence's)
    float* kd = t == 0 ? seqs[t].kc + layer_off + (size_t)pos * dim : ks + (size_t)(t - 1) * dim;
    float* vd = t == 0 ? seqs[t].vc + layer_off + (size_t)pos * dim : vs + (size_t)(t - 1) * dim;
    float* q = Q + (size_t)t * dim;
    float* k = Kr + (size_t)t * dim;
    const float* v = V + (size_t)t * dim;
    const int i = j % (head_size / 2);
    const float fcr = fr[(size_t)pos * (head_size / 2) + i], fci = fi[(size_t)pos * (head_size / 2) + i];
    const float q0 = q[2 * j], q1 = q[2 * j + 1];
    const float a0 = q0 * fcr - q1 * fci, a1 = q0 * fci + q1 * fcr;
    q[2 * j] = a0; q[2 * j + 1] = a1;
    const float k0 = k[2 * j], k1 = k[2 * j + 1];
    const float b0 = k0 * fcr - k1 * fci, b1 = k0 * fci + k1 * fcr;
    k[2 * j] = b0; k[2 * j + 1] = b1;
    kd[2 * j] = b0; kd[2 * j + 1] = b1;                           // infer.rs:32
    vd[2 * j] = v[2 * j]; vd[2 * j + 1] = v[2 * j + 1];           // infer.rs:33
}

// The same for one level of a DRAFT MODEL's tree (q8_spec_model_tree.hpp): the rows of a pass are the nodes of one depth, so the store
// row is the NODE's -- nibble `depth` of the row's path, row node - 1 --, not the pass row's.  A row of depth 0 (the root, the catch-up row in
// front of it) writes its cache row.  ks / vs: the layer's slice of the draft tree store, n_rows - 1 rows; a node is at most n_rows - 1.
__global__ void q8_rope_tree_node_kernel(float* Q, float* Kr, const float* V, const float* fr, const float* fi, int dim, int head_size,
                                         const SeqSlot* seqs, size_t layer_off, float* ks, float* vs, const TreeAnc* anc) {
    RAMA_NO_CONTRACT
    const int j = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (j >= dim / 2) return;
    const int pos = seqs[t].pos;
    if (pos < 0) return;                   // an idle row: nothing rotated, nothing stored
    const int depth = anc[t].depth;
    const int node = (int)((anc[t].path >> (4 * depth)) & 15ull);
    float* kd = depth == 0 ? seqs[t].kc + layer_off + (size_t)pos * dim : ks + (size_t)(node - 1) * dim;
    float* vd = depth == 0 ? seqs[t].vc + layer_off + (size_t)pos * dim : vs + (size_t)(node - 1) * dim;
    float* q = Q + (size_t)t * dim;
    float* k = Kr + (size_t)t * dim;
    const float* v = V + (size_t)t * dim;
    const int i = j % (head_size / 2);
    const float fcr = fr[(size_t)pos * (head_size / 2) + i], fci = fi[(size_t)pos * (head_size / 2) + i];
    const float q0 = q[2 * j], q1 = q[2 * j + 1];
    const float a0 = q0 * fcr - q1 * fci, a1 = q0 * fci + q1 * fcr;
    q[2 * j] = a0; q[2 * j + 1] = a1;
    const float k0 = k[2 * j], k1 = k[2 * j + 1];
    const float b0 = k0 * fcr - k1 * fci, b1 = k0 * fci + k1 * fcr;
    k[2 * j] = b0; k[2 * j + 1] = b1;
    kd[2 * j] = b0; kd[2 * j + 1] = b1;                           // infer.rs:32
    vd[2 * j] = v[2 * j]; vd[2 * j + 1] = v[2 * j + 1];           // infer.rs:33
}

}  // namespace rama
