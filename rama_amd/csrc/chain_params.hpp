// chain_params.hpp -- the parameter blocks, epilogue / norm codes and LDS sizes of chain.hpp's kernels: what a translation unit needs to fill in a
// launch and hand it to chain_api.hip's launchers (ctx.hpp).  Types and constexpr functions only, so it holds no kernel;
// what the fields and sizes mean is told where the kernels are, in chain.hpp.
#pragma once

#include "kernels.hpp"          // Ctl, SeqSlot

namespace rama {

constexpr int kLeadSlots = 2 * 256 + 2;       // tagged words of the leader-workgroup norms: two per layer of a stage (<= 256 layers), one for the final norm
constexpr int kNormMax = 16384;               // the longest vector rmsnorm_chain_kernel / softmax_chain_kernel take

// ---------------------------------------------------------------- cpu.rs:127-153 matmul on chain-order weights (gemv_chain_kernel)
enum { CEPI_STORE = 0, CEPI_RESID = 1, CEPI_QKV = 2, CEPI_SWIGLU = 3 };
enum { CNORM_NONE = 0, CNORM_EXACT = 1, CNORM_TREE = 2, CNORM_LEAD = 3 };      // how the rmsnorm in front of the product is folded in (chain.hpp)

struct ChainParams {
    const float* w[3];     // chain-order matrices (nmat <= 3), each [ceil(rows/16)*16, K]
    float* o[3];           // STORE: o[0]; RESID: o[0] = the product (xb2 / xb); QKV: q, k, v; SWIGLU: o[0] = hb, o[1] = hb2
    const float* x;        // [K] activations, row-major
    const float* nw;       // NORM: rmsnorm gain [K]; x is then the residual stream and the kernel normalises it itself
    float* resid;          // RESID: resid[r] += product (infer.rs:37,47)
    int K, rows, nmat;     // SWIGLU: rows = 2 * hidden (interleaved W1 | W3)
    const Ctl* ctl; int pos_val;
    const float* fr; const float* fi; int head_size;
    float* kc; float* vc;  // this layer's cache slabs [seq, dim]
    // CNORM_LEAD: workgroup 0 of the launch forms v = 1 / sqrt(sum(x^2) / K + 1e-5) (the sum in index order) and publishes it as ONE tagged word;
    // the others request their weights, then wait for it (handoff.hpp's put_tagged, layer_fused.hpp's epoch / error word)
    // ([r5] measured and not kept, profiles/r05_experiments.md: 16 copies of the word on different channels -1.8 %; the leader's compute unit kept free of
    // other workgroups and its waves at priority 3: the word is there 1.1-2 us earlier, the launch no shorter)
    unsigned long long* lead; const unsigned* epoch; unsigned long long* err;
    // half_from > 0 ([r5] one wave per row group): the row groups from this index on are walked as TWO workgroups of 8 rows each (lanes 0..31; the
    // chain-order block of 16 rows is two halves of 512 bytes).  A compute unit streams ~28 GB/s whatever the rest of the chip does, so a launch whose
    // row groups do not divide by the compute units ends when the CUs with one group more are through: llama2-7B's W1|W3 is 1 376 groups on 256 CUs,
    // six on 96 of them and five on the rest; with the last 96 groups as 192 halves it is five and a half at most.
    int half_from;
    float* xout;           // CNORM_LEAD: the leader also stores the normalised vector here (a Device::rmsnorm recorded in front of the run, rama_api.hip flush_mm)
    int lane_reduce;       // [r6] the order of cpu.rs:148 `v.reduce_add()`: LANES_PAIRWISE | LANES_STRIDED | LANES_SEQUENTIAL (ref_order.hpp; "lane_reduce")
};

// XD = activation blocks read ahead from LDS.  Dynamic LDS: K + chain_pad_floats(W, D, XD) floats.
__host__ __device__ constexpr int chain_pad_floats(int W, int D, int XD) { return 16 * ((W + 1) * D + XD); }   // everything the x ring can touch

// ---------------------------------------------------------------- token batches in the reference's order (gemm_chain_kernel)
struct GemmChainParams {
    const float* w[3];      // chain-order matrices (nmat <= 3), each [ceil(rows / 16) * 16, K]
    int nmat, K, rows;      // SWIGLU: rows = 2 * hidden (interleaved W1 | W3)
    const float* x; int xstride;          // activations [n_tok][xstride], row-major
    float* o[3]; int ostride;             // STORE / RESID: o[0][t][row] (RESID: may be NULL); QKV: q = o[0]; SWIGLU: hb = o[0][t][row / 2]
    float* resid; int rstride;            // RESID: resid[t][row] += product (infer.rs:37,47)
    int n_tok;
    int pos0; const float* fr; const float* fi; int head_size; float* kc; float* vc;      // QKV: token t sits at pos0 + t; this layer's cache slabs
    const SeqSlot* seqs; size_t layer_off;   // QKV, independent sequences: token t at seqs[t].pos, its caches at seqs[t].kc / .vc + layer_off
                                             // (every epilogue: the launch returns at once when seqs[0].pos < 0 -- an idle tile of the serving chain, chain.hpp)
    int lane_reduce;        // [r6] as ChainParams::lane_reduce
};
constexpr int kGcWaves = 4, kGcThreads = kGcWaves * 64;
constexpr int kGcBlocks = 8;             // blocks of 16 floats per chunk (8 KiB of weights; 32 KiB of LDS per workgroup at 16 tokens: four workgroups per CU)
constexpr int kGcSets = 2;               // chunks in flight in registers
constexpr int kGcMaxTok = 8 * kGcWaves;  // tokens per weight pass
__host__ __device__ constexpr size_t gemm_chain_lds_bytes(int tpw) { return 2 * ((size_t)kGcBlocks * 1024 + (size_t)(kGcWaves * tpw) * kGcBlocks * 64); }

// ---------------------------------------------------------------- cpu.rs:23-52 multi_head_attention (attention_chain_kernel and the spread form)
constexpr int kAttTile = 64;
constexpr int kAttPiece = 32;                 // floats of a row per staged piece
constexpr int kAttStride = kAttPiece + 4;     // row pitch of a staged piece (16-byte aligned, conflict-free row reads)
__host__ __device__ constexpr size_t attn_chain_region_floats(int head_size, int nw) {
    return (size_t)(nw * 64 * kAttStride) > (size_t)(2 * kAttTile * head_size) ? (size_t)(nw * 64 * kAttStride) : (size_t)(2 * kAttTile * head_size);
}
__host__ __device__ constexpr size_t attn_chain_lds_floats(int head_size, int seq_len, int nw) {
    return (size_t)((head_size + 3) & ~3) + (size_t)seq_len + (size_t)(seq_len >> 5) + 4 + (size_t)((seq_len + 3) & ~3) + attn_chain_region_floats(head_size, nw);
}
// the value tiles are loaded with 8 x 16 bytes per thread
__host__ __device__ constexpr bool attn_chain_fits(int head_size, int nw) { return kAttTile * (head_size / 4) <= (nw >= 16 ? 4 : 8) * 64 * nw; }
__host__ __device__ constexpr size_t attn_fused_values_lds_floats(int seq_len) { return (size_t)seq_len + ((size_t)seq_len >> 5) + 4 + (((size_t)seq_len + 3) & ~(size_t)3); }

}  // namespace rama
