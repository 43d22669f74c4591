// batch_api.hip -- the entries that push many tokens through a layer together: the MFMA token batch (rama_prefill, rama_decode_batch), its
// parity-mode twin, the chained batch (rama_decode_batch_begin* / _steps / _tokens / _stream_poll) and the fp32 serving chain (rama_serve_*).
// Every kernel of prefill_mfma.hpp, prefill_attn.hpp and serve_tile_guard.hpp lives in this translation unit's code object; parity mode's kernels, the samplers, the
// serving chain's tables and the one-token forward are reached through ctx.hpp's launchers and the public entries (DESIGN.md "Translation units").
#include "../../include/rama_hip.h"
#include "kernels.hpp"
#include "prefill_mfma.hpp"
#include "prefill_attn.hpp"
#include "ref_order.hpp"
#include "serve_tile_guard.hpp"
#include "ctx.hpp"

#if defined(RAMA_CHAIN_HPP) || defined(RAMA_LAYER_FUSED_HPP)
#error "batch_api.hip must not include chain.hpp, topp_pick.hpp, layer_fused.hpp or attn_wo.hpp: their kernels belong to chain_api.hip's and rama_api.hip's code objects, and stage_fused_kernel's attributes are set on rama_api.hip's copy"
#endif

#include <algorithm>
#include <cstring>
#include <utility>

using namespace rama;

extern "C" const float* rama_internal_tiled_lookup(const float* src);                    // model.hip
extern "C" const float* rama_internal_chain_lookup(const float* a, int rows, int K);     // model.hip
extern "C" int rama_internal_model_ensure(rama_ctx* ctx, const rama_weights* w, int what);       // model.hip: 1 = chain order, 2 = tile order

// ---- token-batch passes on the matrix cores (prefill_mfma.hpp): up to kMfMaxTok tokens -- the forced
// prompt positions of one sequence (rama_prefill) or one token of each of several independent
// sequences (rama_decode_batch) -- go through a layer together, every weight row streamed once.

// One GEMM launch.  A unit = (row group, K-slice); the launch is cut into one even round over the CUs
// (the kernels hold one 8-wave workgroup per CU), consecutive units of a workgroup prefetching across
// their boundary.  ksplit > 1 only for EPI_STORE, whose K-slices land in slabs the next rmsnorm folds.
template <int RT, int EPI>
static int launch_mf(rama_ctx* c, MfParams& p, int pt) {
    constexpr bool across = EPI == EPI_QKV || EPI == EPI_SWIGLU;
    const int groups = (p.rows + (across ? 16 : 16 * RT) - 1) / (across ? 16 : 16 * RT);
    const int total = groups * p.ksplit;
    p.nunit = std::max(1, (total + std::max(1, c->cu_count) - 1) / std::max(1, c->cu_count));
    const dim3 grid((total + p.nunit - 1) / p.nunit), block(kMfThreads);
    if (p.tiled) {      // p.w[] point at the model's tile-order copies: contiguous 1-KiB weight reads, no lane permute
        if (pt == 1) hipLaunchKernelGGL((gemm_mfma_rows<1, RT, EPI, 2, 3>), grid, block, 0, c->stream, p);
        else if (pt == 2) hipLaunchKernelGGL((gemm_mfma_rows<2, RT, EPI, 2, 3>), grid, block, 0, c->stream, p);
        // MIX (loads scheduled into the MFMA stream) where tools/pf_mfma_bench.hip measures it faster: same arithmetic, same bits
        else if (pt <= 4) hipLaunchKernelGGL((gemm_mfma_rows<4, RT, EPI, 2, 3, 0, (EPI == EPI_QKV || EPI == EPI_STORE) ? 2 : 0>), grid, block, 0, c->stream, p);
        // 65 .. 128 tokens: one K-block per step; as many token tiles as the pass has (a pass of 70 positions pays for 80, not 128)
        else if (pt == 5) hipLaunchKernelGGL((gemm_mfma_rows<5, RT, EPI, 1, 3, 0, EPI == EPI_QKV ? 2 : 0>), grid, block, 0, c->stream, p);
        else if (pt == 6) hipLaunchKernelGGL((gemm_mfma_rows<6, RT, EPI, 1, 3, 0, EPI == EPI_QKV ? 2 : 0>), grid, block, 0, c->stream, p);
        else if (pt == 7) hipLaunchKernelGGL((gemm_mfma_rows<7, RT, EPI, 1, 3, 0, EPI == EPI_QKV ? 2 : 0>), grid, block, 0, c->stream, p);
        else hipLaunchKernelGGL((gemm_mfma_rows<8, RT, EPI, 1, 3, 0, EPI == EPI_QKV ? 2 : 0>), grid, block, 0, c->stream, p);
    } else {
        REQUIRE(pt <= 4, RAMA_EUNSUP, "token batch: more than 64 tokens per pass need the tile-order weight copy");
        if (pt == 1) hipLaunchKernelGGL((gemm_mfma_rows<1, RT, EPI>), grid, block, 0, c->stream, p);
        else if (pt == 2) hipLaunchKernelGGL((gemm_mfma_rows<2, RT, EPI>), grid, block, 0, c->stream, p);
        else hipLaunchKernelGGL((gemm_mfma_rows<4, RT, EPI>), grid, block, 0, c->stream, p);
    }
    LAUNCHCHK();
    return 0;
}

// n token ids -- and, with seqs_dev, the sequence table of n independent sequences: cache bases and position of each, nothing produced yet --
// to the device through the context's pinned staging buffer: the caller's arrays may be gone before the copies run.  Synchronises first,
// after which the pinned buffer is free again.
int stage_tokens(rama_ctx* c, int* toks_dev, const int32_t* tokens_host, int n, SeqSlot* seqs_dev, const rama_run_state* states, const int32_t* pos_host) {
    REQUIRE(n >= 1 && n <= kMfMaxTok, RAMA_EINVAL, "token batch: more tokens than the staging buffer holds");
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(c->pinned_tok, tokens_host, sizeof(int) * n);
    HIPCHK(hipMemcpyAsync(toks_dev, c->pinned_tok, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    if (!seqs_dev) return 0;
    SeqSlot* slots = reinterpret_cast<SeqSlot*>(c->pinned_tok + kMfMaxTok);
    for (int i = 0; i < n; i++) { slots[i].kc = states[i].key_cache; slots[i].vc = states[i].value_cache; slots[i].pos = pos_host[i]; slots[i].pad = 0; }
    HIPCHK(hipMemcpyAsync(seqs_dev, slots, sizeof(SeqSlot) * n, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// row i of the logits slab lg [n, V] to sequence i's run state
int copy_out_logits(rama_ctx* c, const rama_run_state* states, const float* lg, int n, int V) {
    for (int i = 0; i < n; i++)
        HIPCHK(hipMemcpyAsync(states[i].logits, lg + (size_t)i * V, sizeof(float) * V, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// p.w[0..n) = layer li of the given row-major tensors, or of their tile-order copies when the model has them all
static void mf_weights(const rama_ctx* c, MfParams& p, int n, const float* const* base, size_t per_layer, size_t li) {
    const float* t[3] = {nullptr, nullptr, nullptr};
    bool all = c->tune_tiled != 0;
    for (int i = 0; i < n && all; i++) { t[i] = rama_internal_tiled_lookup(base[i]); all = t[i] != nullptr; }
    for (int i = 0; i < n; i++) p.w[i] = (all ? t[i] : base[i]) + li * per_layer;
    p.tiled = all ? 1 : 0;
}

// K-slices of the Wo / W2 products: enough (row group, slice) units to give every CU one, while a
// slice still feeds the workgroup's 8 waves two steps each (16 blocks of 16 floats per wave-step pair)
static int mf_ksplit(const rama_ctx* c, int rows, int K) {
    const int groups = (rows + 31) / 32;
    int ks = 1;
    while (ks < 4 && groups * ks < c->cu_count && K / (ks * 2) >= 512) ks *= 2;
    return ks;
}

// scratch of a pass (tile layout, kMfMaxTok tokens): X residual stream, XN its rmsnorm, Q, XB, HB
// [hidden], SL = up to 4 K-slice slabs [dim]; then token ids, the sequence table, and (decode_batch)
// row-major logits [kMfMaxTok, vocab]
struct BatchScratch { float *X, *XN, *Q, *XB, *HB, *SL, *LG, *SSP; size_t slab; int* toks; SeqSlot* seqs; };
static int regrow_scratch(rama_ctx* c, float** blob, size_t* floats, size_t need) {      // pf_blob / pc_blob is too small: nothing may still read it, then a larger one takes its place
    if (*blob) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(*blob)); *blob = nullptr; *floats = 0; }
    HIPCHK(hipMalloc(blob, need * sizeof(float)));
    *floats = need;
    return 0;
}

static int ensure_batch_scratch(rama_ctx* c, const rama_config* cfg, bool with_logits, BatchScratch* b) {
    const size_t T = kMfMaxTok, dim = cfg->dim, hidden = cfg->hidden_dim;
    const size_t ints = T + (sizeof(SeqSlot) / sizeof(int)) * T;      // token ids [T], then the sequence table [T]
    const size_t ssp = (T / 16) * kRmsParts * 16;        // partial sums of squares per (tile, part, token)
    const size_t need = T * (8 * dim + hidden) + ssp + ints + 64 + (with_logits ? T * (size_t)cfg->vocab_size : 0);
    if (need > c->pf_floats) {
        const int rg = regrow_scratch(c, &c->pf_blob, &c->pf_floats, need);
        destroy_graph(c->bc.cg);      // the chained-batch graph has the old scratch pointers baked in: it must not be replayed on freed memory (the stream is idle by now)
        c->bc.graph_bucket = -1;
        if (rg) return rg;
        // stale tokens of a partly filled 16-token tile flow through the GEMMs as extra columns (never stored): keep them finite
        HIPCHK(hipMemsetAsync(c->pf_blob, 0, need * sizeof(float), c->stream));
    }
    b->slab = T * dim;
    b->X = c->pf_blob; b->XN = b->X + T * dim; b->Q = b->XN + T * dim; b->XB = b->Q + T * dim;
    b->SL = b->XB + T * dim; b->HB = b->SL + 4 * T * dim;
    b->SSP = b->HB + T * hidden;
    b->toks = reinterpret_cast<int*>(b->SSP + ssp);
    b->seqs = reinterpret_cast<SeqSlot*>(b->toks + T);
    b->LG = reinterpret_cast<float*>(b->toks + ints + 64);      // ints is a multiple of 4: 16-byte aligned
    return 0;
}

// b.XN = rmsnorm(b.X += the nslab pending K-slices in b.SL) * gain, per token (prefill_mfma.hpp)
// With tune_norm_in_gemm (default) this is ONE launch: b.XN = b.X * gain, and the GEMM that consumes
// b.XN scales its outputs per token from the partial sums in b.SSP (MfParams::ssp = norm_ssp(c, b)).
static int launch_rmsnorm_tile(rama_ctx* c, const BatchScratch& b, const float* gain, int dim, int ntile, int nslab) {
    if (c->tune_norm_in_gemm) {
        hipLaunchKernelGGL(rms_fold_kernel, dim3(ntile, kRmsParts), dim3(kRmsFoldWaves * 64), 0, c->stream, b.X, b.SSP, dim, (const float*)b.SL, nslab, b.slab, b.XN, gain);
        LAUNCHCHK();
        return 0;
    }
    hipLaunchKernelGGL(rms_fold_kernel, dim3(ntile, kRmsParts), dim3(kRmsFoldWaves * 64), 0, c->stream, b.X, b.SSP, dim, (const float*)b.SL, nslab, b.slab, (float*)nullptr, (const float*)nullptr);
    LAUNCHCHK();
    hipLaunchKernelGGL(rms_scale_kernel, dim3(ntile, kRmsParts), dim3(256), 0, c->stream, b.XN, (const float*)b.X, gain, (const float*)b.SSP, dim);
    LAUNCHCHK();
    return 0;
}
static const float* norm_ssp(const rama_ctx* c, const BatchScratch& b) { return c->tune_norm_in_gemm ? b.SSP : nullptr; }

// tokens (prefill) / sequences (decode_batch) one weight pass can take: 128 when every matrix it streams has its
// tile-order copy (8 token tiles per wave need the contiguous 1-KiB weight reads), else 64
static int mf_pass_cap(const rama_ctx* c, const rama_weights* w, bool with_cls) {
    const float* ms[8] = {w->wq, w->wk, w->wv, w->wo, w->w1, w->w2, w->w3, w->wcls};
    bool all = c->tune_tiled != 0;
    for (int i = 0; i < (with_cls ? 8 : 7) && all; i++) all = rama_internal_tiled_lookup(ms[i]) != nullptr;
    return all ? kMfMaxTok : kMfMaxTokRows;
}

static bool mf_shape_ok(const rama_config* cfg) { return cfg->dim % 16 == 0 && cfg->hidden_dim % 16 == 0; }
static int mf_pt(int ntile) { return ntile <= 1 ? 1 : (ntile == 2 ? 2 : (ntile <= 4 ? 4 : ntile)); }      // launch_mf's PT for a pass of ntile 16-token tiles

// nt <= kMfMaxTok tokens (already embedded in b.X, tile layout) through every layer.
// seqs == false: consecutive positions p0.. of ONE sequence (its cache bases key_cache / value_cache);
// seqs == true: token t belongs to independent sequence t (device table b.seqs).
// tmax = the longest context any token of the pass attends to (timesteps): sizes the attention scratch.
// On return the residual stream is b.X + the *nslab_out K-slices in b.SL (folded by the caller).
static int run_layers_batched(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const BatchScratch& b,
                              int nt, int p0, float* key_cache, float* value_cache, bool seqs, int tmax, int* nslab_out) {
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads;
    const size_t dd = (size_t)dim * dim, hd = (size_t)hidden * dim;
    const int ntile = (nt + 15) / 16, pt = mf_pt(ntile);
    const int ks_wo = mf_ksplit(c, dim, dim), ks_w2 = mf_ksplit(c, dim, hidden);
    int pending = 0;      // K-slices of the previous product waiting in b.SL
    int rc;
    for (int layer = 0; layer < cfg->n_layers; layer++) {
        const size_t li = (size_t)layer;
        const size_t layer_off = li * cfg->seq_len * dim;
        MfParams p{};
        p.n_tok = nt; p.ksplit = 1; p.slab_floats = b.slab;
        // infer.rs:19 (+ the residual add of the previous layer's W2 product, :47)
        rc = launch_rmsnorm_tile(c, b, w->rms_att_weight + li * dim, dim, ntile, pending); if (rc) return rc;
        // infer.rs:20-33: Wq | Wk | Wv, RoPE, cache append
        { const float* bs[3] = {w->wq, w->wk, w->wv}; mf_weights(c, p, 3, bs, dd, li); }
        p.x = b.XN; p.o = b.Q; p.K = dim; p.rows = dim; p.ssp = norm_ssp(c, b);
        p.pos0 = p0; p.fr = w->freq_cis_real; p.fi = w->freq_cis_imag; p.head_size = hs;
        p.kc = key_cache ? key_cache + layer_off : nullptr; p.vc = value_cache ? value_cache + layer_off : nullptr;
        p.seqs = seqs ? b.seqs : nullptr; p.layer_off = layer_off;
        rc = launch_mf<3, EPI_QKV>(c, p, pt); if (rc) return rc;
        {   // infer.rs:34: query z attends to positions 0..pos(z)
            AttnParams a{};
            a.q = b.Q; a.kc = p.kc; a.vc = p.vc; a.att = nullptr; a.xb = b.XB; a.ctl = nullptr; a.pos_val = p0;
            a.dim = dim; a.head_size = hs; a.seq_len = cfg->seq_len; a.tiled = 1;
            a.seqs = seqs ? b.seqs : nullptr; a.layer_off = layer_off;
            const int G = attn_group_width(hs);
            dim3 grid(cfg->n_heads, 1, nt);
            const bool tiles = !seqs && c->tune_prefill_attn && (hs == 16 || hs == 32 || hs == 48 || hs == 64 || hs == 128);
            if (tiles) {            // one sequence: 16 queries per workgroup share every cache row (prefill_attn.hpp)
                const dim3 tg(cfg->n_heads, ntile);
#define RAMA_TILE_ATTN(W_) do { \
                    if (hs == 16) hipLaunchKernelGGL((attention_tile_mfma_kernel<1, W_>), tg, dim3(W_ * 64), 0, c->stream, a, nt); \
                    else if (hs == 32) hipLaunchKernelGGL((attention_tile_mfma_kernel<2, W_>), tg, dim3(W_ * 64), 0, c->stream, a, nt); \
                    else if (hs == 48) hipLaunchKernelGGL((attention_tile_mfma_kernel<3, W_>), tg, dim3(W_ * 64), 0, c->stream, a, nt); \
                    else if (hs == 64) hipLaunchKernelGGL((attention_tile_mfma_kernel<4, W_>), tg, dim3(W_ * 64), 0, c->stream, a, nt); \
                    else hipLaunchKernelGGL((attention_tile_mfma_kernel<8, W_>), tg, dim3(W_ * 64), 0, c->stream, a, nt); } while (0)
                if (tmax >= 512) RAMA_TILE_ATTN(8);     // long contexts: 8 waves share the key tiles
                else RAMA_TILE_ATTN(4);
#undef RAMA_TILE_ATTN
            } else
            // scores scratch: tmax = the longest context of the pass (timesteps)
            if (tmax <= 256) {      // short contexts: 4-wave workgroups, 8 of them per CU
                size_t shm = (size_t)(attn_scratch_floats(G, 4) + tmax) * sizeof(float);
                if (G == 16) hipLaunchKernelGGL((attention_kernel<16, false, 4>), grid, dim3(256), shm, c->stream, a);
                else if (G == 32) hipLaunchKernelGGL((attention_kernel<32, false, 4>), grid, dim3(256), shm, c->stream, a);
                else hipLaunchKernelGGL((attention_kernel<64, false, 4>), grid, dim3(256), shm, c->stream, a);
            } else {
                size_t shm = (size_t)(attn_scratch_floats(G) + tmax) * sizeof(float);
                REQUIRE(shm <= 64 * 1024, RAMA_EUNSUP, "token batch: context too long for the single-workgroup attention kernel");
                if (G == 16) hipLaunchKernelGGL((attention_kernel<16, false>), grid, dim3(kAttnThreads), shm, c->stream, a);
                else if (G == 32) hipLaunchKernelGGL((attention_kernel<32, false>), grid, dim3(kAttnThreads), shm, c->stream, a);
                else hipLaunchKernelGGL((attention_kernel<64, false>), grid, dim3(kAttnThreads), shm, c->stream, a);
            }
            LAUNCHCHK();
        }
        // infer.rs:35: Wo . xb as K-slices; the residual add (:37) rides in the next rmsnorm
        { const float* bs[1] = {w->wo}; mf_weights(c, p, 1, bs, dd, li); }
        p.x = b.XB; p.o = b.SL; p.K = dim; p.rows = dim; p.ksplit = ks_wo; p.ssp = nullptr;
        rc = launch_mf<2, EPI_STORE>(c, p, pt); if (rc) return rc;
        // infer.rs:37,39
        rc = launch_rmsnorm_tile(c, b, w->rms_ffn_weight + li * dim, dim, ntile, ks_wo); if (rc) return rc;
        // infer.rs:41-45: W1 | W3, SiLU * gate
        { const float* bs[2] = {w->w1, w->w3}; mf_weights(c, p, 2, bs, hd, li); }
        p.x = b.XN; p.o = b.HB; p.K = dim; p.rows = hidden; p.ksplit = 1; p.ssp = norm_ssp(c, b);
        rc = launch_mf<2, EPI_SWIGLU>(c, p, pt); if (rc) return rc;
        // infer.rs:46: W2 . hb as K-slices (:47 rides in the next rmsnorm / the caller's fold)
        { const float* bs[1] = {w->w2}; mf_weights(c, p, 1, bs, hd, li); }
        p.x = b.HB; p.o = b.SL; p.K = hidden; p.rows = dim; p.ksplit = ks_w2; p.ssp = nullptr;
        rc = launch_mf<2, EPI_STORE>(c, p, pt); if (rc) return rc;
        pending = ks_w2;
    }
    *nslab_out = pending;
    return 0;
}

// ---- parity mode: the forced prompt positions in the reference's rounding order, 32 per weight pass (chain.hpp
// gemm_chain_kernel).  Every position's cache rows are what its own forward() writes, bit for bit: the same chains per
// output, the same exact sums in the norms and the softmax, the same attention per (head, position).  The LAST position
// then goes through forward() itself, which leaves the run state (x, xb, q, .., logits) exactly as the reference's loop
// does (mod.rs:187-194).  *done = false: shape or copies not available, nothing was enqueued.

// the layers of one pass of nt <= 16 tokens whose residual rows sit in b.X: consecutive positions p0.. of one sequence
// (key_cache / value_cache its cache bases), or -- seqs != NULL -- token t of independent sequence t (device table)
struct ChainBatch { float *X, *XN, *Q, *XB, *HB, *ATT; const float *cq, *ck, *cv, *co, *c13, *c2; int nw; size_t att_lds; };
// tile: the rows are a tile of the serving chain's row table (serve_pass below) -- every launch gets the table, and returns at once when the tile's first row is idle
static int chain_batch_layers(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const ChainBatch& b, int nt, int p0,
                              float* key_cache, float* value_cache, const SeqSlot* seqs, bool tile = false) {
    const SeqSlot* tseqs = tile ? seqs : nullptr;
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads, H = cfg->n_heads, seq = cfg->seq_len;
    const size_t dd = (size_t)dim * dim, hd = (size_t)hidden * dim;
    int rc;
    for (int layer = 0; layer < cfg->n_layers; layer++) {
        const size_t li = (size_t)layer, layer_off = li * seq * dim;
        float* kc = key_cache ? key_cache + layer_off : nullptr;
        float* vc = value_cache ? value_cache + layer_off : nullptr;
        rc = launch_rmsnorm_chain(c, b.XN, b.X, w->rms_att_weight + li * dim, dim, nullptr, nt, dim, tseqs); if (rc) return rc;      // infer.rs:19
        {   // :20-33
            GemmChainParams p{};
            p.w[0] = b.cq + li * dd; p.w[1] = b.ck + li * dd; p.w[2] = b.cv + li * dd; p.nmat = 3; p.K = dim; p.rows = dim;
            p.x = b.XN; p.xstride = dim; p.o[0] = b.Q; p.ostride = dim; p.n_tok = nt;
            p.pos0 = p0; p.fr = w->freq_cis_real; p.fi = w->freq_cis_imag; p.head_size = hs; p.kc = kc; p.vc = vc;
            p.seqs = seqs; p.layer_off = layer_off;
            rc = launch_gemm_chain(c, p, CEPI_QKV); if (rc) return rc;
        }
        {   // :34, one workgroup per (head, token)
            RefAttnParams a{};
            a.q = b.Q; a.kc = kc; a.vc = vc; a.att = b.ATT; a.xb = b.XB; a.ctl = nullptr; a.pos_val = p0;
            a.dim = dim; a.head_size = hs; a.seq_len = seq; a.tok_stride = dim; a.att_stride = H * seq;
            a.seqs = seqs; a.layer_off = layer_off;
            rc = launch_attention_chain_tokens(c, a, H, nt, b.nw, b.att_lds); if (rc) return rc;
        }
        {   // :35-37
            GemmChainParams p{};
            p.w[0] = b.co + li * dd; p.nmat = 1; p.K = dim; p.rows = dim; p.x = b.XB; p.xstride = dim; p.n_tok = nt;
            p.resid = b.X; p.rstride = dim; p.seqs = tseqs;
            rc = launch_gemm_chain(c, p, CEPI_RESID); if (rc) return rc;
        }
        rc = launch_rmsnorm_chain(c, b.XN, b.X, w->rms_ffn_weight + li * dim, dim, nullptr, nt, dim, tseqs); if (rc) return rc;      // :39
        {   // :41-45
            GemmChainParams p{};
            p.w[0] = b.c13 + li * 2 * hd; p.nmat = 1; p.K = dim; p.rows = 2 * hidden; p.x = b.XN; p.xstride = dim; p.n_tok = nt;
            p.o[0] = b.HB; p.ostride = hidden; p.seqs = tseqs;
            rc = launch_gemm_chain(c, p, CEPI_SWIGLU); if (rc) return rc;
        }
        {   // :46-47
            GemmChainParams p{};
            p.w[0] = b.c2 + li * hd; p.nmat = 1; p.K = hidden; p.rows = dim; p.x = b.HB; p.xstride = hidden; p.n_tok = nt;
            p.resid = b.X; p.rstride = dim; p.seqs = tseqs;
            rc = launch_gemm_chain(c, p, CEPI_RESID); if (rc) return rc;
        }
    }
    return 0;
}
// infer.rs:49-51 for n rows: normed = rmsnorm(src) * gain in one launch, logits [n, vocab] = Wcls . normed over the classifier's chain-order copy, kGcMaxTok rows per weight pass
static int chain_classifier(rama_ctx* c, const rama_config* cfg, const float* gain, const float* ccls, const float* src, float* normed, float* logits, int n) {
    const int dim = cfg->dim, V = cfg->vocab_size;
    int rc = launch_rmsnorm_chain(c, normed, src, gain, dim, nullptr, n, dim); if (rc) return rc;
    for (int r0 = 0; r0 < n; r0 += kGcMaxTok) {
        GemmChainParams p{};
        p.w[0] = ccls; p.nmat = 1; p.K = dim; p.rows = V; p.x = normed + (size_t)r0 * dim; p.xstride = dim; p.o[0] = logits + (size_t)r0 * V; p.ostride = V; p.n_tok = std::min(kGcMaxTok, n - r0);
        rc = launch_gemm_chain(c, p, CEPI_STORE); if (rc) return rc;
    }
    return 0;
}

// shape check, chain-order copies and scratch of the parity-mode token batches.  *ok = false: not available for this
// shape / these weights (the caller falls back to one forward() per token).  Scratch, row-major per token: X residual
// stream, XN its norm, Q, XB attention output, HB; att rows; token ids; the sequence table; (with_logits) LG [16][vocab]
struct ChainScratch { ChainBatch b; int* toks; SeqSlot* seqs; float* LG; const float* ccls; };
// the part that sizes nothing: the shape check, the chain-order copies (made when the model has none yet) and the attention's geometry -- b's weight
// pointers, nw and att_lds, *ccls.  (the serving chain has rows of its own and asks for this alone)
static int chain_batch_copies(rama_ctx* c, const rama_config* cfg, const rama_weights* w, bool with_logits, ChainBatch* b, const float** ccls_out, bool* ok) {
    *ok = false;
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads, seq = cfg->seq_len, V = cfg->vocab_size;
    if (!c->tune_chain || !c->tune_prefill_chain || dim % 16 || hidden % 16 || dim > 16000 || hidden > 16000 || !attn_chain_ok(hs, seq)) return 0;
    if (!rmsnorm_chain_ok((size_t)dim)) return 0;
    int rc = ensure_chain_copy(c, cfg, w, nullptr); if (rc) return rc;
    const float* cq = rama_internal_chain_lookup(w->wq, dim, dim), *ck = rama_internal_chain_lookup(w->wk, dim, dim);
    const float* cv = rama_internal_chain_lookup(w->wv, dim, dim), *co = rama_internal_chain_lookup(w->wo, dim, dim);
    const float* c13 = rama_internal_chain_lookup(w->w1, 2 * hidden, dim), *c2 = rama_internal_chain_lookup(w->w2, dim, hidden);
    const float* ccls = with_logits ? rama_internal_chain_lookup(w->wcls, V, dim) : nullptr;
    if (!cq || !ck || !cv || !co || !c13 || !c2 || (with_logits && !ccls)) return 0;
    const int nw = attn_chain_waves(hs, false);
    const size_t att_lds = attn_chain_lds_bytes(hs, seq, nw);
    REQUIRE(att_lds <= kAttnChainMaxLds, RAMA_EUNSUP, "token batch (parity mode): context too long for the score buffer");
    *b = ChainBatch{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, cq, ck, cv, co, c13, c2, nw, att_lds};
    *ccls_out = ccls;
    *ok = true;
    return 0;
}
static int chain_batch_setup(rama_ctx* c, const rama_config* cfg, const rama_weights* w, bool with_logits, ChainScratch* out, bool* ok) {
    const int dim = cfg->dim, hidden = cfg->hidden_dim, H = cfg->n_heads, seq = cfg->seq_len, V = cfg->vocab_size;
    ChainBatch cb{};
    const float* ccls = nullptr;
    int rc = chain_batch_copies(c, cfg, w, with_logits, &cb, &ccls, ok); if (rc || !*ok) return rc;
    *ok = false;
    const size_t T = kGcMaxTok;
    const size_t slot_floats = (sizeof(SeqSlot) * T + sizeof(float) - 1) / sizeof(float);
    const size_t need = T * (4 * (size_t)dim + hidden) + T * (size_t)H * seq + 64 + slot_floats + 4 + (with_logits ? T * (size_t)V : 0);
    if (need > c->pc_floats) { rc = regrow_scratch(c, &c->pc_blob, &c->pc_floats, need); if (rc) return rc; }
    float* X = c->pc_blob, *XN = X + T * dim, *Q = XN + T * dim, *XB = Q + T * dim, *HB = XB + T * dim, *ATT = HB + T * hidden;
    out->toks = reinterpret_cast<int*>(ATT + T * (size_t)H * seq);
    out->seqs = reinterpret_cast<SeqSlot*>(out->toks + 64);                       // 8-byte aligned: every term above is a multiple of 16 floats
    out->LG = reinterpret_cast<float*>(out->toks + 64) + slot_floats + 4 - ((slot_floats) & 3);      // 16-byte aligned
    out->ccls = ccls;
    cb.X = X; cb.XN = XN; cb.Q = Q; cb.XB = XB; cb.HB = HB; cb.ATT = ATT;
    out->b = cb;
    *ok = true;
    return 0;
}

static int prefill_chain(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                         const int32_t* tokens_host, int n_tokens, int pos0, bool* done) {
    *done = false;
    if (n_tokens < 2) return 0;
    const int dim = cfg->dim;
    ChainScratch sc{};
    int rc = chain_batch_setup(c, cfg, w, false, &sc, done); if (rc || !*done) return rc;
    float* X = sc.b.X; int* toks = sc.toks;
    const ChainBatch& cb = sc.b;
    c->embedded_x = nullptr; c->host_pos = -1;
    const int n_batch = n_tokens - 1;                             // the last position runs as forward()
    for (int c0 = 0; c0 < n_batch; c0 += kGcMaxTok) {
        const int nt = std::min(kGcMaxTok, n_batch - c0), p0 = pos0 + c0;
        rc = stage_tokens(c, toks, tokens_host + c0, nt); if (rc) return rc;
        hipLaunchKernelGGL(embed_rows_kernel, dim3((dim + 255) / 256, nt), dim3(256), 0, c->stream, X, w->token_embedding_table, (const int*)toks, nt, dim);
        LAUNCHCHK();
        rc = chain_batch_layers(c, cfg, w, cb, nt, p0, s->key_cache, s->value_cache, nullptr); if (rc) return rc;
    }
    return rama_forward(c, cfg, w, s, tokens_host[n_tokens - 1], pos0 + n_tokens - 1);
}

// rama_decode_batch in parity mode: the sequences share every weight pass, 32 at a time, through the same kernels; each
// sequence's appended cache rows and its logits are bit for bit those of its own forward().  (x / xb / q .. of the states
// are not maintained -- the call's contract, see the header.)
static int decode_batch_chain(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_run_state* states,
                              const int32_t* tokens_host, const int32_t* pos_host, int n_seq, bool* done) {
    *done = false;
    const int dim = cfg->dim, V = cfg->vocab_size;
    if (n_seq < 2) return 0;
    ChainScratch sc{};
    int rc = chain_batch_setup(c, cfg, w, true, &sc, done); if (rc || !*done) return rc;
    c->embedded_x = nullptr; c->host_pos = -1;
    for (int c0 = 0; c0 < n_seq; c0 += kGcMaxTok) {
        const int nt = std::min(kGcMaxTok, n_seq - c0);
        rc = stage_tokens(c, sc.toks, tokens_host + c0, nt, sc.seqs, states + c0, pos_host + c0); if (rc) return rc;
        hipLaunchKernelGGL(embed_rows_kernel, dim3((dim + 255) / 256, nt), dim3(256), 0, c->stream, sc.b.X, w->token_embedding_table, (const int*)sc.toks, nt, dim);
        LAUNCHCHK();
        rc = chain_batch_layers(c, cfg, w, sc.b, nt, 0, nullptr, nullptr, sc.seqs); if (rc) return rc;
        rc = chain_classifier(c, cfg, w->rms_final_weight, sc.ccls, sc.b.X, sc.b.XN, sc.LG, nt); if (rc) return rc;
        rc = copy_out_logits(c, states + c0, sc.LG, nt, V); if (rc) return rc;
    }
    return 0;
}

int rama_prefill(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                 const int32_t* tokens_host, int n_tokens, int pos0) {
    RAMA_ENTER(c);
    REQUIRE(c && tokens_host, RAMA_EINVAL, "prefill: NULL argument");
    int rc = check_cfg(cfg); if (rc) return rc;
    rama_stage st{0, cfg->n_layers, 1, 1};
    rc = check_stage(cfg, w, s, &st); if (rc) return rc;
    REQUIRE(n_tokens >= 1 && pos0 >= 0 && pos0 + n_tokens <= cfg->seq_len, RAMA_EINVAL, "prefill: positions outside [0, seq_len)");
    for (int i = 0; i < n_tokens; i++) REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < cfg->vocab_size, RAMA_EINVAL, "prefill: token outside the vocabulary");
    if (set_device(c)) return 1;
    const int dim = cfg->dim;
    if (c->tune_ref_order) {      // parity mode: the chain-order token-batch kernels when the shape and the copies allow
        bool done = false;
        rc = prefill_chain(c, cfg, w, s, tokens_host, n_tokens, pos0, &done);
        if (rc || done) return rc;
    }
    if (c->tune_ref_order || !mf_shape_ok(cfg) || !attn_one_wg_holds(dim / cfg->n_heads, pos0 + n_tokens)) {
        // reference-order mode; widths that are not whole 16-float blocks, or contexts the one-workgroup attention cannot
        // hold: the reference's own schedule, one forward() per forced token (mod.rs:187-194)
        for (int i = 0; i < n_tokens; i++) { rc = rama_forward(c, cfg, w, s, tokens_host[i], pos0 + i); if (rc) return rc; }
        return 0;
    }
    BatchScratch b{};
    if (c->tune_tiled) { rc = rama_internal_model_ensure(c, w, 2); if (rc) return rc; }
    rc = ensure_batch_scratch(c, cfg, false, &b); if (rc) return rc;
    c->embedded_x = nullptr; c->host_pos = -1;
    int last_nt = 0, nslab = 0;
    // positions per weight pass: 128 when every layer matrix has its tile-order copy, else 64
    const int per_pass = std::min(c->tune_prefill_tok, mf_pass_cap(c, w, false));
    for (int c0 = 0; c0 < n_tokens; c0 += per_pass) {
        const int nt = std::min(per_pass, n_tokens - c0), p0 = pos0 + c0;
        last_nt = nt;
        rc = stage_tokens(c, b.toks, tokens_host + c0, nt); if (rc) return rc;
        hipLaunchKernelGGL(embed_tile_kernel, dim3((dim / 4 + 255) / 256, nt), dim3(256), 0, c->stream, b.X, w->token_embedding_table, (const int*)b.toks, nt, dim);
        LAUNCHCHK();
        rc = run_layers_batched(c, cfg, w, b, nt, p0, s->key_cache, s->value_cache, false, p0 + nt, &nslab);
        if (rc) return rc;
    }
    // the last position's residual stream (+ the last W2 product), then infer.rs:49-51 for it only
    // (generate() ignores the logits of the forced positions before it)
    hipLaunchKernelGGL(untile_fold_kernel, dim3((dim / 4 + 255) / 256, 1), dim3(256), 0, c->stream, s->x, (const float*)b.X, last_nt - 1, dim,
                       (const float*)b.SL, nslab, b.slab);
    LAUNCHCHK();
    return launch_classifier(c, s->logits, w->wcls, s->x, w->rms_final_weight, dim, cfg->vocab_size);
}

// One pass for the n_seq sequences of the device tables b.toks / b.seqs: embedding rows, every layer, final norm and
// the classifier as one more GEMM into b.LG [n_seq, vocab] (row-major).  tmax bounds the longest context (score buffers).
static int enqueue_batch_pass(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const BatchScratch& b, int n_seq, int tmax) {
    const int dim = cfg->dim, V = cfg->vocab_size;
    hipLaunchKernelGGL(embed_tile_kernel, dim3((dim / 4 + 255) / 256, n_seq), dim3(256), 0, c->stream, b.X, w->token_embedding_table, (const int*)b.toks, n_seq, dim);
    LAUNCHCHK();
    int nslab = 0;
    int rc = run_layers_batched(c, cfg, w, b, n_seq, 0, nullptr, nullptr, true, tmax, &nslab);
    if (rc) return rc;
    // infer.rs:49-51 for every sequence: fold the last product, final rmsnorm, classifier
    const int ntile = (n_seq + 15) / 16;
    rc = launch_rmsnorm_tile(c, b, w->rms_final_weight, dim, ntile, nslab); if (rc) return rc;
    MfParams p{};
    p.n_tok = n_seq; p.ksplit = 1; { const float* bs[1] = {w->wcls}; mf_weights(c, p, 1, bs, 0, 0); }
    p.x = b.XN; p.o = b.LG; p.o_stride = V; p.K = dim; p.rows = V; p.ssp = norm_ssp(c, b);
    return launch_mf<2, EPI_STORE_ROWS>(c, p, mf_pt(ntile));
}

// ---- one decode step for up to kMfMaxTok INDEPENDENT sequences (the server's concurrent requests,
// SURVEY 8e): every weight row is streamed once for all of them.  No reference counterpart; the
// contract is "what forward(token_i, pos_i) leaves in state_i, for every i": cache rows + logits.
int rama_decode_batch(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_run_state* states,
                      const int32_t* tokens_host, const int32_t* pos_host, int n_seq) {
    RAMA_ENTER(c);
    REQUIRE(c && states && tokens_host && pos_host, RAMA_EINVAL, "decode_batch: NULL argument");
    REQUIRE(n_seq >= 1 && n_seq <= kMfMaxTok, RAMA_EINVAL, "decode_batch: 1..128 sequences per call");
    int rc = check_cfg(cfg); if (rc) return rc;
    rama_stage st{0, cfg->n_layers, 1, 1};
    if (set_device(c)) return 1;
    if (c->tune_tiled && !c->tune_ref_order && n_seq > kMfMaxTokRows) { rc = rama_internal_model_ensure(c, w, 2); if (rc) return rc; }
    REQUIRE(n_seq <= kMfMaxTokRows || c->tune_ref_order || mf_pass_cap(c, w, true) >= n_seq, RAMA_EINVAL,
            "decode_batch: more than 64 sequences per call need a resident model's tile-order weight copies");
    for (int i = 0; i < n_seq; i++) {
        rc = check_stage(cfg, w, &states[i], &st); if (rc) return rc;
        REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < cfg->vocab_size, RAMA_EINVAL, "decode_batch: token outside the vocabulary");
        REQUIRE(pos_host[i] >= 0 && pos_host[i] < cfg->seq_len, RAMA_EINVAL, "decode_batch: position outside [0, seq_len)");
        for (int j = 0; j < i; j++) REQUIRE(states[j].key_cache != states[i].key_cache && states[j].logits != states[i].logits, RAMA_EINVAL, "decode_batch: two sequences share a run state");
    }
    const int dim = cfg->dim, V = cfg->vocab_size;
    int tmax = 1;
    for (int i = 0; i < n_seq; i++) tmax = std::max(tmax, pos_host[i] + 1);
    if (c->tune_ref_order) {      // parity mode: the chain-order token-batch kernels when the shape and the copies allow
        bool done = false;
        rc = decode_batch_chain(c, cfg, w, states, tokens_host, pos_host, n_seq, &done);
        if (rc || done) return rc;
    }
    if (c->tune_ref_order || !mf_shape_ok(cfg) || V % 4 != 0 || !attn_one_wg_holds(dim / cfg->n_heads, tmax)) {   // see rama_prefill: one forward() per sequence
        for (int i = 0; i < n_seq; i++) {
            rama_run_state si = states[i];
            rc = rama_forward(c, cfg, w, &si, tokens_host[i], pos_host[i]); if (rc) return rc;
        }
        return 0;
    }
    BatchScratch b{};
    if (c->tune_tiled) { rc = rama_internal_model_ensure(c, w, 2); if (rc) return rc; }
    rc = ensure_batch_scratch(c, cfg, true, &b); if (rc) return rc;
    c->embedded_x = nullptr; c->host_pos = -1;
    rc = stage_tokens(c, b.toks, tokens_host, n_seq, b.seqs, states, pos_host); if (rc) return rc;
    rc = enqueue_batch_pass(c, cfg, w, b, n_seq, tmax);
    if (rc) return rc;
    return copy_out_logits(c, states, b.LG, n_seq, V);
}

// ---- the same pass CHAINED ON THE DEVICE: every sequence's (token, position) lives in device memory, a step ends with
// one argmax per sequence that writes the next token and advances the position, and a step is one hipGraph replay --
// no per-sequence download, no host round trip per step (rama_decode_batch costs one call and n_seq 4-byte downloads
// per step when the tokens are fed back through the host).
// per_seq == nullptr: the greedy chain (argmax_batch_kernel); else every step ends in the batched top-p sampler.  Every argument is
// checked before anything of the previous chain is touched.
static int batch_begin(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_run_state* states,
                       const int32_t* tokens_host, const int32_t* pos_host, int n_seq, int max_steps, const rama_seq_sampling* per_seq) {
    REQUIRE(c && states && tokens_host && pos_host, RAMA_EINVAL, "decode_batch_begin: NULL argument");
    REQUIRE(n_seq >= 1 && n_seq <= kMfMaxTok, RAMA_EINVAL, "decode_batch_begin: 1..128 sequences");
    REQUIRE(max_steps >= 1 && max_steps <= (1 << 20), RAMA_EINVAL, "decode_batch_begin: bad max_steps");
    int rc = check_cfg(cfg); if (rc) return rc;
    REQUIRE(mf_shape_ok(cfg) && cfg->vocab_size % 4 == 0 && !c->tune_ref_order, RAMA_EUNSUP,
            "decode_batch_begin: needs dim, hidden_dim multiples of 16, vocab_size a multiple of 4, fast mode");
    rama_stage st{0, cfg->n_layers, 1, 1};
    if (set_device(c)) return 1;
    if (c->tune_tiled && n_seq > kMfMaxTokRows) { rc = rama_internal_model_ensure(c, w, 2); if (rc) return rc; }
    REQUIRE(n_seq <= kMfMaxTokRows || mf_pass_cap(c, w, true) >= n_seq, RAMA_EINVAL,
            "decode_batch_begin: more than 64 sequences need a resident model's tile-order weight copies");
    int pmax = 0;
    for (int i = 0; i < n_seq; i++) {
        rc = check_stage(cfg, w, &states[i], &st); if (rc) return rc;
        REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < cfg->vocab_size, RAMA_EINVAL, "decode_batch_begin: token outside the vocabulary");
        REQUIRE(pos_host[i] >= 0 && pos_host[i] + max_steps <= cfg->seq_len, RAMA_EINVAL, "decode_batch_begin: position + max_steps beyond seq_len");
        for (int j = 0; j < i; j++) REQUIRE(states[j].key_cache != states[i].key_cache, RAMA_EINVAL, "decode_batch_begin: two sequences share a run state");
        pmax = std::max(pmax, pos_host[i]);
    }
    size_t n_forced_all = 0;
    if (per_seq) {
        REQUIRE(cfg->vocab_size <= kToppBlock * kToppMaxBlocks, RAMA_EUNSUP, "decode_batch_begin_sampled: vocab_size above 32768");
        for (int i = 0; i < n_seq; i++) {
            const rama_seq_sampling& q = per_seq[i];
            REQUIRE(topp_params_ok(q.temperature, q.topp, q.u), RAMA_EINVAL, "decode_batch_begin_sampled: temperature >= 0, topp in [0,1], u in [0,1)");
            REQUIRE(q.n_forced >= 0 && (q.n_forced == 0 || q.forced), RAMA_EINVAL, "decode_batch_begin_sampled: bad forced list");
            for (int k = 0; k < q.n_forced; k++)
                REQUIRE(q.forced[k] >= 0 && q.forced[k] < cfg->vocab_size, RAMA_EINVAL, "decode_batch_begin_sampled: forced token outside the vocabulary");
            n_forced_all += (size_t)q.n_forced;
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    auto& bc = c->bc;
    drop_graph(c);
    if (!bc.toks) { HIPCHK(hipMalloc(&bc.toks, sizeof(int) * kMfMaxTok)); HIPCHK(hipMalloc(&bc.seqs, sizeof(SeqSlot) * kMfMaxTok)); }
    if (bc.out_cap < max_steps) {
        hipFree(bc.out); bc.out = nullptr;
        if (bc.ring) { hipHostFree(bc.ring); bc.ring = nullptr; }
        HIPCHK(hipMalloc(&bc.out, sizeof(int) * (size_t)kMfMaxTok * max_steps));
        HIPCHK(hipHostMalloc(&bc.ring, sizeof(int) * (size_t)kMfMaxTok * max_steps, hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&bc.ring_dev), bc.ring, 0));
        bc.out_cap = max_steps;
    }
    memset(bc.ring, 0, sizeof(int) * (size_t)kMfMaxTok * bc.out_cap);      // (the stream was drained above: nothing is on its way)
    rc = stage_tokens(c, bc.toks, tokens_host, n_seq, bc.seqs, states, pos_host); if (rc) return rc;
    bc.sampled = per_seq != nullptr;
    if (per_seq) {
        // the sampling records and the forced lists go to the device once; a step reads them there
        if (!bc.rows) HIPCHK(hipMalloc(&bc.rows, sizeof(ToppRow) * kMfMaxTok));
        if (bc.forced_cap < n_forced_all) {
            hipFree(bc.forced); bc.forced = nullptr; bc.forced_cap = 0;
            HIPCHK(hipMalloc(&bc.forced, sizeof(int) * n_forced_all));
            bc.forced_cap = n_forced_all;
        }
        ToppRow rows[kMfMaxTok];
        size_t at = 0;
        for (int i = 0; i < n_seq; i++) {
            const rama_seq_sampling& q = per_seq[i];
            rows[i] = ToppRow{q.temperature, q.topp, q.u, q.n_forced, q.n_forced ? bc.forced + at : nullptr};
            if (q.n_forced) HIPCHK(hipMemcpy(bc.forced + at, q.forced, sizeof(int) * q.n_forced, hipMemcpyHostToDevice));
            at += (size_t)q.n_forced;
        }
        HIPCHK(hipMemcpy(bc.rows, rows, sizeof(ToppRow) * n_seq, hipMemcpyHostToDevice));
        rc = ensure_topp_batch(c, n_seq, cfg->vocab_size); if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    bc.n_seq = n_seq; bc.pos_max = pmax; bc.steps_done = 0; bc.cfg = *cfg; bc.w = *w;
    if (c->tune_tiled) { rc = rama_internal_model_ensure(c, w, 2); if (rc) return rc; }
    BatchScratch b{};
    return ensure_batch_scratch(c, cfg, true, &b);
}

int rama_decode_batch_begin(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_run_state* states,
                            const int32_t* tokens_host, const int32_t* pos_host, int n_seq, int max_steps) {
    RAMA_ENTER(c);
    return batch_begin(c, cfg, w, states, tokens_host, pos_host, n_seq, max_steps, nullptr);
}

int rama_decode_batch_begin_sampled(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_run_state* states,
                                    const int32_t* tokens_host, const int32_t* pos_host, int n_seq, int max_steps,
                                    const rama_seq_sampling* per_seq) {
    RAMA_ENTER(c);
    REQUIRE(per_seq, RAMA_EINVAL, "decode_batch_begin_sampled: per_seq is NULL");
    return batch_begin(c, cfg, w, states, tokens_host, pos_host, n_seq, max_steps, per_seq);
}

// what ends a chained batch step: one argmax per sequence, or the batched top-p sampler (forced / temperature-0 rows included)
static int enqueue_batch_finish(rama_ctx* c, const BatchScratch& b) {
    auto& bc = c->bc;
    const int V = bc.cfg.vocab_size;
    if (!bc.sampled) {
        BatchArgmaxParams ap{b.LG, V, bc.toks, bc.seqs, bc.out, bc.out_cap, bc.ring_dev};
        hipLaunchKernelGGL(argmax_batch_kernel, dim3(bc.n_seq), dim3(1024), 0, c->stream, ap);
        LAUNCHCHK();
        return 0;
    }
    ToppBatchParams fin{};
    fin.toks = bc.toks; fin.seqs = bc.seqs; fin.out = bc.out; fin.out_cap = bc.out_cap; fin.ring = bc.ring_dev;
    return enqueue_topp_batch(c, bc.rows, bc.n_seq, b.LG, (size_t)V, V, fin);
}

int rama_decode_batch_steps(rama_ctx* c, int n_steps) {
    RAMA_ENTER(c);
    REQUIRE(c && c->bc.n_seq > 0, RAMA_EINVAL, "decode_batch_steps: call rama_decode_batch_begin first");
    REQUIRE(n_steps >= 0 && c->bc.steps_done + n_steps <= c->bc.out_cap, RAMA_EINVAL, "decode_batch_steps: more steps than rama_decode_batch_begin allowed for");
    if (set_device(c)) return 1;
    auto& bc = c->bc;
    const rama_config* cfg = &bc.cfg;
    BatchScratch b{};
    int rc = ensure_batch_scratch(c, cfg, true, &b); if (rc) return rc;
    b.toks = bc.toks; b.seqs = bc.seqs;                           // the chain's own cursors, not the scratch of a single pass
    c->embedded_x = nullptr; c->host_pos = -1;
    for (int i = 0; i < n_steps; i++) {
        // the score buffers are sized by the longest context: one graph per bucket of 256 timesteps
        const int tmax = bc.pos_max + 1, bucket = (tmax + 255) / 256;
        if (!c->graph_mode) {
            rc = enqueue_batch_pass(c, cfg, &bc.w, b, bc.n_seq, bucket * 256); if (rc) return rc;
            rc = enqueue_batch_finish(c, b); if (rc) return rc;
        } else {
            if (bc.graph_bucket != bucket) {
                bc.graph_bucket = -1;
                rc = capture_graph(c, bc.cg, [&] {
                    const int re = enqueue_batch_pass(c, cfg, &bc.w, b, bc.n_seq, bucket * 256);
                    return re ? re : enqueue_batch_finish(c, b);
                });
                if (rc) return rc;
                bc.graph_bucket = bucket;
            }
            rc = replay_graph(c, bc.cg); if (rc) return rc;
        }
        bc.pos_max++; bc.steps_done++;
    }
    return 0;
}

int rama_decode_batch_tokens(rama_ctx* c, int32_t* out_host, int max_per_seq, int* n_per_seq) {
    RAMA_ENTER(c);
    REQUIRE(c && out_host && n_per_seq && c->bc.n_seq > 0, RAMA_EINVAL, "decode_batch_tokens: bad argument");
    auto& bc = c->bc;
    const int n = std::min(bc.steps_done, max_per_seq);
    HIPCHK(hipStreamSynchronize(c->stream));
    { const int rh = handoff_check(c); if (rh) return rh; }
    for (int s_ = 0; s_ < bc.n_seq && n > 0; s_++)
        HIPCHK(hipMemcpy(out_host + (size_t)s_ * max_per_seq, bc.out + (size_t)s_ * bc.out_cap, sizeof(int) * n, hipMemcpyDeviceToHost));
    *n_per_seq = n;
    return 0;
}

// tokens `from`.. sequence `seq` of the chained batch has produced so far, without touching the stream (the host-visible
// ring of rama_decode_stream_poll, one row per sequence): a server hands each request its tokens as they appear
int rama_decode_batch_stream_poll(rama_ctx* c, int seq, int from, int32_t* out_host, int max_tokens, int* n_ready) {
    RAMA_ENTER(c);
    REQUIRE(c && n_ready && c->bc.n_seq > 0 && c->bc.ring && seq >= 0 && seq < c->bc.n_seq && from >= 0 && max_tokens >= 0 && (max_tokens == 0 || out_host),
            RAMA_EINVAL, "decode_batch_stream_poll: bad argument");
    *n_ready = read_ring(c->bc.ring + (size_t)seq * c->bc.out_cap, c->bc.out_cap, from, out_host, max_tokens);
    return 0;
}

// ---- THE SERVING CHAIN IN PARITY MODE (rama_serve_*): continuous batching for an fp32 model in the reference's rounding order.  The
// tables, the scheduler, the gather, the admission and the pick are the Q8 serving chain's (q8_serve.hpp, reached through ctx.hpp's launchers and the
// shared host layer of q8_serve_api.hip); the pass is chain_batch_layers over the step's row table in TILES of kGcMaxTok rows, in ascending order -- a slot's
// prompt rows may straddle a tile boundary, and the later tile's attention reads the cache rows the earlier tile's pass wrote.  Idle rows come last in
// the table: a tile whose first row is idle costs its launches and no weight pass (chain.hpp).

static void serve_release(rama_ctx* c) {
    auto& sv = c->sv;
    destroy_graph(sv.cg);
    serve_state_free(sv);
    hipFree(sv.scratch); hipFree(sv.tguard);
    sv = rama_ctx::Serve();
}
// drop_graph of rama_api.hip: the chained batch's step and the serving chain's (each captured again by its next _steps call)
void drop_batch_graphs(rama_ctx* c) {
    destroy_graph(c->bc.cg);
    c->bc.graph_bucket = -1;
    destroy_graph(c->sv.cg);
}
// rama_ctx_destroy: everything this translation unit allocates; the stream is idle and not yet destroyed
void release_batch(rama_ctx* c) {
    hipFree(c->pf_blob); hipFree(c->pc_blob);
    hipFree(c->bc.toks); hipFree(c->bc.seqs); hipFree(c->bc.out); if (c->bc.ring) hipHostFree(c->bc.ring);
    hipFree(c->bc.rows); hipFree(c->bc.forced);
    serve_release(c);
}
// rama_state_free: the run state of a slot whose occupant the host cannot yet see DONE ends the chain
void serve_state_gone(rama_ctx* c, const rama_run_state* s) {
    auto& sv = c->sv;
    if (!sv.n_slots || !serve_state_uses(sv, s)) return;
    (void)hipStreamSynchronize(c->stream);
    destroy_graph(sv.cg);
    sv.live = false;
}
// model.hip: the tensors in [base, base + n) are about to be freed -- a chain over them is dead
extern "C" void rama_internal_serve_weights_gone(rama_ctx* c, const float* base, size_t n) {
    if (!c || !c->sv.n_slots || !base) return;
    const float* q = c->sv.w.wq;
    if (q >= base && q < base + n) { destroy_graph(c->sv.cg); c->sv.live = false; }
}

// the pass's rows: one allocation, laid out the same way at begin and at every _steps call
struct ServeScratch { ChainBatch b; float *XG, *XGN, *LG; const float* ccls; size_t floats; };
static ServeScratch serve_scratch(const rama_ctx::Serve& sv, const ChainBatch& copies, const float* ccls) {
    const rama_config& cfg = sv.cfg;
    const size_t R = (size_t)sv.max_rows, N = (size_t)sv.n_slots, dim = (size_t)cfg.dim, hidden = (size_t)cfg.hidden_dim;
    ServeScratch s{};
    s.b = copies;
    float* p = sv.scratch;
    s.b.X = p; p += R * dim; s.b.XN = p; p += R * dim; s.b.Q = p; p += R * dim; s.b.XB = p; p += R * dim;
    s.b.HB = p; p += R * hidden;
    s.b.ATT = p; p += (size_t)kGcMaxTok * (size_t)cfg.n_heads * (size_t)cfg.seq_len;       // one tile's score rows: the tiles run one after the other
    if (!sv.spec) { s.XG = p; p += N * dim; s.XGN = p; p += N * dim; }       // (a chain with drafts classifies the rows where they sit)
    s.LG = p; p += (sv.spec ? R : N) * (size_t)cfg.vocab_size;
    s.ccls = ccls;
    s.floats = (size_t)(p - sv.scratch);
    return s;
}
// A hook for the tests, exported like the other rama_internal_* accessors and not in the header: where the pass keeps its rows
// (X | XN | Q | XB | HB, max_rows rows each) -- tests/test_hip_serve.py fills an idle tile's rows with a sentinel and sees that no step writes them
extern "C" int rama_internal_serve_scratch(rama_ctx* c, float** rows5, int* max_rows) {
    if (!c || !c->sv.n_slots || !rows5 || !max_rows) return RAMA_EINVAL;
    const ServeScratch s = serve_scratch(c->sv, ChainBatch{}, nullptr);
    rows5[0] = s.b.X; rows5[1] = s.b.XN; rows5[2] = s.b.Q; rows5[3] = s.b.XB; rows5[4] = s.b.HB;
    *max_rows = c->sv.max_rows;
    return 0;
}

// ... and its logits rows: [n_slots, vocab] on a plain chain, [max_rows, vocab] on one with drafts -- tests/test_hip_serve_spec.py poisons the rows of a
// tile that carries no logits and sees that the classifier leaves them alone
extern "C" int rama_internal_serve_logits(rama_ctx* c, float** logits, int* rows, int* vocab) {
    if (!c || !c->sv.n_slots || !logits || !rows || !vocab) return RAMA_EINVAL;
    *logits = serve_scratch(c->sv, ChainBatch{}, nullptr).LG;
    *rows = c->sv.spec ? c->sv.max_rows : c->sv.n_slots;
    *vocab = c->sv.cfg.vocab_size;
    return 0;
}

int rama_serve_end(rama_ctx* c) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "serve_end: ctx is NULL");
    if (!c->sv.n_slots && !c->sv.blob) return 0;
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    serve_release(c);
    return 0;
}

// rama_serve_begin (spec false) and rama_serve_begin_spec: the latter sizes the drafting tables as well, and its sampler and logits for max_rows rows
// dcfg, dw (rama_serve_begin_model): a chain with drafts whose drafts are that Q8 model's -- the sampler for the first draft pass's 2 n_slots rows as
// well, and the draft side's allocations (serve_model_alloc)
static int serve_begin(rama_ctx* c, const rama_config* cfg, const rama_weights* w, int n_slots, int max_rows, int max_new_cap, bool spec, int n_draft_cap, int hint_cap,
                       const rama_config* dcfg = nullptr, const rama_q8_weights* dw = nullptr) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    int rc = check_cfg(cfg); if (rc) return rc;
    if (dcfg) {
        rc = check_cfg(dcfg); if (rc) return rc;
        rc = serve_model_begin_check("serve_begin_model", cfg, dcfg, dw, n_slots, max_rows, n_draft_cap); if (rc) return rc;
    }
    REQUIRE(w && w->token_embedding_table && w->rms_final_weight && w->wq && w->wcls, RAMA_EINVAL, "serve_begin: missing weights");
    if (!dcfg) { rc = check_slots_rows("serve_begin", n_slots, max_rows); if (rc) return rc; }      // (with a draft model: serve_model_begin_check has looked)
    REQUIRE(max_new_cap >= 1 && max_new_cap <= cfg->seq_len - 1, RAMA_EINVAL, "serve_begin: max_new_cap outside [1, seq_len - 1]");
    REQUIRE(c->tune_ref_order == 1 && !c->tune_tol && !c->tune_bar, RAMA_EUNSUP, "serve_begin: parity mode only (\"ref_order\" = 1): no fast mode, no bar mode");
    const int V = cfg->vocab_size;
    const bool sampler = V > 1 && V <= kToppBlock * kToppMaxBlocks;
    REQUIRE(sampler || V % 4 == 0, RAMA_EUNSUP, "serve_begin: vocab_size % 4 != 0 needs vocab_size <= 32768");
    rc = check_spec_caps("serve_begin_spec", n_draft_cap, hint_cap); if (rc) return rc;      // (before anything is allocated: the copies below may be made here)
    if (set_device(c)) return 1;
    // shape, chain-order copies (made here when the model has none yet), the score buffer: what chain_batch_setup takes.  Nothing of a running chain is touched
    ChainBatch copies{};
    const float* ccls = nullptr;
    bool ok = false;
    rc = chain_batch_copies(c, cfg, w, true, &copies, &ccls, &ok); if (rc) return rc;
    REQUIRE(ok, RAMA_EUNSUP, "serve_begin: a shape or weights the parity-mode token batch does not take (dim, hidden_dim multiples of 16; chain-order copies)");
    if (sampler) { rc = ensure_topp_batch(c, spec ? std::max(max_rows, dcfg ? 2 * n_slots : 0) : n_slots, V); if (rc) return rc; }      // sized here, outside any capture (a chain with drafts picks per row)
    // the new chain is made beside the running one, which goes only when nothing can fail any more
    rama_ctx::Serve fresh;
    auto make = [&]() -> int {
        int rm = serve_state_alloc_spec(c, fresh, cfg->seq_len, n_slots, max_rows, max_new_cap, spec, n_draft_cap, hint_cap); if (rm) return rm;
        fresh.cfg = *cfg; fresh.w = *w; fresh.sampler = sampler;
        if (spec) HIPCHK(hipMalloc(&fresh.tguard, sizeof(SeqSlot) * (size_t)((max_rows + kGcMaxTok - 1) / kGcMaxTok)));
        const size_t floats = serve_scratch(fresh, copies, ccls).floats;
        HIPCHK(hipMalloc(&fresh.scratch, floats * sizeof(float)));
        HIPCHK(hipMemsetAsync(fresh.scratch, 0, floats * sizeof(float), c->stream));      // (an idle row is computed along in a live tile: finite values, never read by anyone)
        HIPCHK(hipStreamSynchronize(c->stream));      // (also: nothing of the previous chain is still running)
        return dcfg ? serve_model_alloc(c, fresh, dcfg, dw) : 0;
    };
    rc = make();
    if (rc) { serve_state_free(fresh); hipFree(fresh.scratch); hipFree(fresh.tguard); return rc; }
    serve_release(c);
    fresh.live = true;
    c->sv = std::move(fresh);
    return 0;
}

int rama_serve_begin(rama_ctx* c, const rama_config* cfg, const rama_weights* w, int n_slots, int max_rows, int max_new_cap) {
    return serve_begin(c, cfg, w, n_slots, max_rows, max_new_cap, false, 0, 0);
}

int rama_serve_begin_spec(rama_ctx* c, const rama_config* cfg, const rama_weights* w, int n_slots, int max_rows, int max_new_cap, int n_draft_cap, int hint_cap) {
    return serve_begin(c, cfg, w, n_slots, max_rows, max_new_cap, true, n_draft_cap, hint_cap);
}

// ---- MODEL DRAFTS INSIDE THE FP32 SERVING CHAIN: rama_serve_begin_spec with hint_cap 0, plus a Q8 draft model over the same vocabulary.
// The tables, the draft passes and the serve_model_* kernels are the Q8 chain's (q8_serve_model.hpp in q8_serve_api.hip's code object, reached through ctx.hpp);
// the verify half is the step of rama_serve_begin_spec.
int rama_serve_begin_model(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_config* dcfg, const rama_q8_weights* dw,
                           int n_slots, int max_rows, int max_new_cap, int n_draft_cap) {
    RAMA_ENTER(c);
    REQUIRE(c && dcfg && dw, RAMA_EINVAL, "serve_begin_model: NULL argument");
    return serve_begin(c, cfg, w, n_slots, max_rows, max_new_cap, true, n_draft_cap, 0, dcfg, dw);
}

// rama_serve_admit (n_cached 0), rama_serve_admit_at and -- spec != NULL -- rama_serve_admit_spec: one body, rama_q8_serve_admit*'s checks in their order.
// The slot starts PROMPT at cursor = n_cached, over rows 0 .. n_cached - 1 that earlier work on the stream has put into the run state's caches
static const ServeNames kServeNames{"serve_admit", "serve_admit_at", "rama_serve_begin", "serve_admit_spec", "rama_serve_begin_spec"};
static int serve_admit(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                       const rama_q8_serve_plan* plan, const rama_q8_serve_spec* spec = nullptr) {
    RAMA_ENTER(c);
    REQUIRE(c && c->sv.n_slots > 0, RAMA_EINVAL, "serve_admit: call rama_serve_begin first");
    auto& sv = c->sv;
    int rc = serve_admit_head(kServeNames, sv, sv.live, slot, state, context_host, plan); if (rc) return rc;
    rama_stage st{0, sv.cfg.n_layers, 1, 1};
    rc = check_stage(&sv.cfg, &sv.w, state, &st); if (rc) return rc;
    rc = serve_admit_tail(kServeNames, sv, sv.cfg, slot, state, context_host, n_context, n_cached, plan); if (rc) return rc;
    rc = serve_admit_spec_check(kServeNames, sv, sv.cfg.vocab_size, spec); if (rc) return rc;
    if (sv.model) {      // a chain begun with rama_serve_begin_model: no lookup drafts, and no run state that a live slot drafts on
        REQUIRE(!spec, RAMA_EINVAL, "serve_admit_spec: the chain was begun with rama_serve_begin_model: model drafts replace the lookup");
        REQUIRE(!serve_model_state_clash(sv, slot, state), RAMA_EINVAL, "serve_admit: the run state is already in a live slot");
    }
    if (set_device(c)) return 1;
    rc = serve_admit_install(c, sv, slot, state, context_host, n_context, n_cached, plan); if (rc) return rc;
    rc = serve_admit_spec_install(c, sv, slot, spec); if (rc) return rc;
    sv.states[slot] = *state; sv.occupied[slot] = 1; sv.gen[slot]++;
    if (sv.model) sv.dstates[slot] = rama_run_state{};
    return 0;
}

int rama_serve_admit(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, const rama_q8_serve_plan* plan) {
    return serve_admit(c, slot, state, context_host, n_context, 0, plan);
}

int rama_serve_admit_at(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                        const rama_q8_serve_plan* plan) {
    return serve_admit(c, slot, state, context_host, n_context, n_cached, plan);
}

int rama_serve_admit_spec(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                          const rama_q8_serve_plan* plan, const rama_q8_serve_spec* spec) {
    REQUIRE(spec, RAMA_EINVAL, "serve_admit_spec: NULL argument");
    return serve_admit(c, slot, state, context_host, n_context, n_cached, plan, spec);
}

static const ServeNames kServeModelNames{"serve_admit_model", "serve_admit_model", "rama_serve_begin_model", "serve_admit_model", "rama_serve_begin_model"};
// rama_q8_serve_admit_model's checks in their order, in this entry's words; the draft run state is a Q8 stack's, the target's an fp32 model's
int rama_serve_admit_model(rama_ctx* c, int slot, const rama_run_state* state, const rama_run_state* dstate, const int32_t* context_host, int n_context,
                           int n_cached, const rama_q8_serve_plan* plan, int n_draft) {
    RAMA_ENTER(c);
    REQUIRE(c && c->sv.n_slots > 0 && c->sv.model, RAMA_EINVAL, "serve_admit_model: call rama_serve_begin_model first");
    auto& sv = c->sv;
    int rc = serve_admit_head(kServeModelNames, sv, sv.live, slot, state, context_host, plan); if (rc) return rc;
    REQUIRE(dstate, RAMA_EINVAL, "serve_admit_model: NULL argument");
    rama_stage st{0, sv.cfg.n_layers, 1, 1};
    rc = check_stage(&sv.cfg, &sv.w, state, &st); if (rc) return rc;
    rc = serve_admit_model_dstate(c, sv, dstate); if (rc) return rc;
    rc = serve_admit_tail(kServeModelNames, sv, sv.cfg, slot, state, context_host, n_context, n_cached, plan); if (rc) return rc;
    rc = serve_admit_model_check(kServeModelNames, sv, slot, state, dstate, n_context, plan, n_draft); if (rc) return rc;
    if (set_device(c)) return 1;
    rc = serve_admit_install(c, sv, slot, state, context_host, n_context, n_cached, plan); if (rc) return rc;
    rc = serve_admit_model_install(c, sv, slot, dstate, n_context, n_draft); if (rc) return rc;
    sv.states[slot] = *state; sv.dstates[slot] = *dstate; sv.occupied[slot] = 1; sv.gen[slot]++;
    return 0;
}

int rama_serve_cancel(rama_ctx* c, const int32_t* slots, int n) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "serve_cancel: ctx is NULL");
    return serve_cancel(c, "serve_cancel", c->sv, slots, n);
}

// the pass over the step's row table, tile by tile in ascending order
static int serve_pass(rama_ctx* c, const ServeScratch& s) {
    auto& sv = c->sv;
    const size_t dim = (size_t)sv.cfg.dim, hidden = (size_t)sv.cfg.hidden_dim;
    for (int r0 = 0; r0 < sv.max_rows; r0 += kGcMaxTok) {
        ChainBatch tb = s.b;
        tb.X += r0 * dim; tb.XN += r0 * dim; tb.Q += r0 * dim; tb.XB += r0 * dim; tb.HB += r0 * hidden;
        const int rc = chain_batch_layers(c, &sv.cfg, &sv.w, tb, std::min(kGcMaxTok, sv.max_rows - r0), 0, nullptr, nullptr, sv.t.rows + r0, true);
        if (rc) return rc;
    }
    return 0;
}
// one step: the scheduler, the wanted rows' embeddings, the pass, the logits of the rows that carry them (infer.rs:49-51 per slot), the pick
static int enqueue_serve_step(rama_ctx* c, const ServeScratch& s) {
    auto& sv = c->sv;
    const int dim = sv.cfg.dim, V = sv.cfg.vocab_size, N = sv.n_slots;
    int rc = launch_serve_schedule(c, sv.t); if (rc) return rc;
    rc = launch_serve_embed(c, s.b.X, sv.w.token_embedding_table, sv.t, dim); if (rc) return rc;
    rc = serve_pass(c, s); if (rc) return rc;
    rc = launch_serve_gather(c, s.XG, s.b.X, sv.t, dim); if (rc) return rc;
    rc = chain_classifier(c, &sv.cfg, sv.w.rms_final_weight, s.ccls, s.XG, s.XGN, s.LG, N); if (rc) return rc;
    return launch_serve_pick(c, sv.t, s.LG, V, sv.sampler);
}

// the verify half of a step with drafts, behind the scheduler: from the tiles' guard entries to the accept rule
static int enqueue_serve_verify(rama_ctx* c, const ServeScratch& s) {
    auto& sv = c->sv;
    const int dim = sv.cfg.dim, V = sv.cfg.vocab_size, R = sv.max_rows;
    int rc;
    hipLaunchKernelGGL(serve_tile_guard_kernel, dim3(1), dim3(kTileGuardThreads), 0, c->stream, (const int*)sv.st.lflag, R, sv.tguard);
    LAUNCHCHK();
    rc = launch_serve_embed(c, s.b.X, sv.w.token_embedding_table, sv.t, dim); if (rc) return rc;
    rc = serve_pass(c, s); if (rc) return rc;
    for (int r0 = 0; r0 < R; r0 += kGcMaxTok) {       // infer.rs:49-51 per tile: a tile without a logits row returns before its first load
        const int nt = std::min(kGcMaxTok, R - r0);
        const SeqSlot* guard = sv.tguard + r0 / kGcMaxTok;
        rc = launch_rmsnorm_chain(c, s.b.XN + (size_t)r0 * dim, s.b.X + (size_t)r0 * dim, sv.w.rms_final_weight, dim, nullptr, nt, dim, guard); if (rc) return rc;
        GemmChainParams p{};
        p.w[0] = s.ccls; p.nmat = 1; p.K = dim; p.rows = V; p.x = s.b.XN + (size_t)r0 * dim; p.xstride = dim; p.o[0] = s.LG + (size_t)r0 * V; p.ostride = V; p.n_tok = nt;
        p.seqs = guard;
        rc = launch_gemm_chain(c, p, CEPI_STORE); if (rc) return rc;
    }
    rc = launch_serve_spec_pick(c, sv.t, sv.st, s.LG, V, sv.sampler); if (rc) return rc;
    return launch_serve_spec_accept(c, sv.t, sv.st);
}

// one step of a chain begun with rama_serve_begin_spec: the drafts, the scheduler, the tiles' guard entries, the wanted rows' embeddings, the pass, then --
// tile by tile, where the rows sit -- the final norm and the classifier of the tiles that hold a logits row, every flagged row's pick, the accept rule
static int enqueue_serve_spec_step(rama_ctx* c, const ServeScratch& s) {
    auto& sv = c->sv;
    int rc = launch_serve_draft(c, sv.t, sv.st); if (rc) return rc;
    rc = launch_serve_spec_schedule(c, sv.t, sv.st); if (rc) return rc;
    return enqueue_serve_verify(c, s);
}
// one step of a chain begun with rama_serve_begin_model: the drafting half is the Q8 chain's (the wants, the scheduler, n_draft_cap passes of the draft
// model with their picks), the verify half the step's above, then the draft cursors
static int enqueue_serve_model_step(rama_ctx* c, const ServeScratch& s) {
    int rc = launch_serve_model_drafts(c, c->sv); if (rc) return rc;
    rc = enqueue_serve_verify(c, s); if (rc) return rc;
    return launch_serve_model_close(c, c->sv);
}
int rama_serve_steps(rama_ctx* c, int n_steps) {
    RAMA_ENTER(c);
    REQUIRE(c && c->sv.n_slots > 0, RAMA_EINVAL, "serve_steps: call rama_serve_begin first");
    auto& sv = c->sv;
    REQUIRE(sv.live, RAMA_EINVAL, "serve_steps: the chain's model or the run state of an occupied slot has been freed");
    REQUIRE(n_steps >= 0, RAMA_EINVAL, "serve_steps: n_steps < 0");
    REQUIRE(c->tune_ref_order == 1 && !c->tune_tol && !c->tune_bar, RAMA_EUNSUP, "serve_steps: the context has left parity mode");
    if (set_device(c)) return 1;
    // the chain-order copies may have been released and made again since the step was captured: it is then captured again
    ChainBatch copies{};
    const float* ccls = nullptr;
    bool ok = false;
    int rc = chain_batch_copies(c, &sv.cfg, &sv.w, true, &copies, &ccls, &ok); if (rc) return rc;
    REQUIRE(ok, RAMA_EUNSUP, "serve_steps: the chain-order copies are gone and cannot be made (\"chain\" / \"prefill_chain\" = 0?)");
    const float* now[7] = {copies.cq, copies.ck, copies.cv, copies.co, copies.c13, copies.c2, ccls};
    if (memcmp(now, sv.copies, sizeof now)) { if (sv.cg.exec) HIPCHK(hipStreamSynchronize(c->stream)); destroy_graph(sv.cg); memcpy(sv.copies, now, sizeof now); }
    if (sv.sampler) { rc = ensure_topp_batch(c, sv.spec ? std::max(sv.max_rows, sv.draft_rows) : sv.n_slots, sv.cfg.vocab_size); if (rc) return rc; }
    const ServeScratch s = serve_scratch(sv, copies, ccls);
    auto step = [&] { return sv.model ? enqueue_serve_model_step(c, s) : sv.spec ? enqueue_serve_spec_step(c, s) : enqueue_serve_step(c, s); };
    c->embedded_x = nullptr; c->host_pos = -1;
    const bool graphs = c->graph_mode && c->kp.kernel_id < 0;
    for (int i = 0; i < n_steps; i++, sv.steps++) {
        if (!graphs) { rc = step(); if (rc) return rc; continue; }
        if (!sv.cg.exec) {
            rc = capture_graph(c, sv.cg, step); if (rc) return rc;
            sv.captures++;
        }
        rc = replay_graph(c, sv.cg); if (rc) return rc;
    }
    return 0;
}

int rama_serve_poll(rama_ctx* c, int slot, int from, int32_t* out_host, int max_tokens, int* n_ready, int* finished, int* generation) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "serve_poll: bad argument");
    return serve_poll_ring("serve_poll", c->sv, slot, from, out_host, max_tokens, n_ready, finished, generation);
}

int rama_serve_tokens(rama_ctx* c, int slot, int32_t* out_host, int max_tokens, int* n_out) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "serve_tokens: bad argument");
    return serve_tokens_back(c, "serve_tokens", c->sv, slot, out_host, max_tokens, n_out);
}

int rama_serve_stats(rama_ctx* c, rama_q8_serve_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->sv.n_slots > 0, RAMA_EINVAL, "serve_stats: bad argument");
    return serve_report(c, c->sv, c->sv.captures, c->sv.spec ? c->sv.st.lflag : nullptr, out);
}

int rama_serve_spec_stats(rama_ctx* c, rama_q8_serve_spec_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->sv.n_slots > 0 && c->sv.spec, RAMA_EINVAL, "serve_spec_stats: no chain begun with rama_serve_begin_spec");
    return serve_spec_report(c, c->sv, out);
}

int rama_serve_model_stats(rama_ctx* c, rama_q8_serve_model_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->sv.n_slots > 0 && c->sv.model, RAMA_EINVAL, "serve_model_stats: no chain begun with rama_serve_begin_model");
    return serve_model_report(c, c->sv, out);
}
