// chain_api.hip -- parity mode's launches and the samplers: every kernel and __device__ global of chain.hpp, topp_pick.hpp and
// topp_kernels.hpp lives in this translation unit's code object, and with them the host code that launches them -- the chain-order
// matvecs, norms and attention (one token and token batches), the top-p samplers (one row and batched) and their C entries.  The other
// translation units fill in chain_params.hpp's parameter blocks and call the launchers that ctx.hpp declares (DESIGN.md "Translation units").
#include "ctx.hpp"
#include "chain.hpp"
#include "q8_tree.hpp"          // attention_tree_kernel (after chain.hpp: its attention half)
#include "topp_pick.hpp"
#include "topp_kernels.hpp"

#include <algorithm>

// The kernels that ask for more than the 64 KiB of dynamic LDS a kernel gets by default.  An attribute reaches the kernel copy of the
// translation unit that sets it, so these are set here, where the kernels are launched.
// (parity mode's attention keeps two product tiles + the scores of a whole context in LDS)
int chain_api_init(rama_ctx*) {
    HIPCHK(hipFuncSetAttribute((const void*)attention_chain_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_chain_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_chain_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_tree_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_tree_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_tree_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_draft_tree_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_draft_tree_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
    HIPCHK(hipFuncSetAttribute((const void*)attention_draft_tree_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnChainMaxLds));
#define RAMA_GC_ATTR(TPW_) \
    HIPCHK(hipFuncSetAttribute((const void*)gemm_chain_kernel<TPW_, CEPI_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_chain_lds_bytes(TPW_))); \
    HIPCHK(hipFuncSetAttribute((const void*)gemm_chain_kernel<TPW_, CEPI_RESID>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_chain_lds_bytes(TPW_))); \
    HIPCHK(hipFuncSetAttribute((const void*)gemm_chain_kernel<TPW_, CEPI_QKV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_chain_lds_bytes(TPW_))); \
    HIPCHK(hipFuncSetAttribute((const void*)gemm_chain_kernel<TPW_, CEPI_SWIGLU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_chain_lds_bytes(TPW_)));
    RAMA_GC_ATTR(1) RAMA_GC_ATTR(2) RAMA_GC_ATTR(4) RAMA_GC_ATTR(8)
#undef RAMA_GC_ATTR
    return 0;
}

// diagnostics (not in the C ABI header): how often the one-pass exact sum (chain.hpp seq_sum_predict) held / fell back
extern "C" int rama_internal_pred_stats(rama_ctx* c, unsigned* held, unsigned* fell_back, int reset) {
    RAMA_ENTER(c);
    unsigned h[2] = {0, 0};
    hipStreamSynchronize(c->stream);
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(rama::g_pred_stats), sizeof h) != hipSuccess) return 1;
    if (held) *held = h[0];
    if (fell_back) *fell_back = h[1];
    if (reset) { const unsigned z[2] = {0, 0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rama::g_pred_stats), z, sizeof z) != hipSuccess) return 1; }
    return 0;
}

// test entry (not in the C ABI header): seqsum_fast.hpp's sum of a_dev[0..n) on nw waves; out_dev[0..3] = sum, held, items, 100 MHz ticks
extern "C" int rama_internal_seqsum_fast(rama_ctx* c, const float* a_dev, int n, int nw, float* out_dev) {
    RAMA_ENTER(c);
    REQUIRE(c && a_dev && out_dev && n > 0, RAMA_EINVAL, "seqsum_fast: bad argument");
    const int per = (n + 64 * nw - 1) / (64 * nw);
#define RAMA_FS(NW_, R_) hipLaunchKernelGGL((seqsum_fast_test_kernel<NW_, R_>), dim3(1), dim3(NW_ * 64), 0, c->stream, a_dev, n, out_dev)
#define RAMA_FS_R(NW_) do { if (per <= 8) RAMA_FS(NW_, 8); else if (per <= 16) RAMA_FS(NW_, 16); else if (per <= 32) RAMA_FS(NW_, 32); else if (per <= 64) RAMA_FS(NW_, 64); \
                            else return fail(RAMA_EINVAL, "seqsum_fast: list too long for this many waves", __FILE__, __LINE__); } while (0)
    if (nw == 1) RAMA_FS_R(1); else if (nw == 2) RAMA_FS_R(2); else if (nw == 4) RAMA_FS_R(4);
    else return fail(RAMA_EINVAL, "seqsum_fast: nw must be 1, 2 or 4", __FILE__, __LINE__);
#undef RAMA_FS_R
#undef RAMA_FS
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------- parity mode at streaming speed (chain.hpp)

// W waves per 16 rows, D blocks per wave in flight: by how many row groups share a CU (few groups -> more waves
// and deeper rings per group, so that >= ~128 KiB per CU are on the way); tune_chain_d = 100 W + D overrides
// norm: how the rmsnorm in front of the product is folded in when p.nw is given -- CNORM_EXACT (parity mode, narrow models: the exact
// sequential sum by lane ripples, K <= 1024), CNORM_TREE (tolerance mode: a tree-shaped sum, K <= 8192)
static bool chain_norm_fits(int K, int norm) { return K % 16 == 0 && K <= (norm == CNORM_TREE ? 8192 : 1024); }
template <int EPI>
static int launch_chain_epi(rama_ctx* c, ChainParams& p, int norm) {
    REQUIRE(p.K % 16 == 0 && p.K > 0 && p.rows > 0, RAMA_EINVAL, "chain-order matvec: width must be a multiple of 16");
    REQUIRE((p.nw != nullptr) == (norm != CNORM_NONE), RAMA_EINVAL, "chain-order matvec: a folded norm needs its gain vector");
    const int groups = p.nmat * ((p.rows + 15) / 16);
    p.lane_reduce = c->tune_lane_reduce;
    int W, D;
    if (c->tune_chain_d > 0) { W = c->tune_chain_d / 100; D = c->tune_chain_d % 100; }
    else if (EPI == CEPI_RESID && norm == CNORM_NONE && c->tune_chain_resid_d > 0) { W = c->tune_chain_resid_d / 100; D = c->tune_chain_resid_d % 100; }
    else if (EPI == CEPI_RESID && norm == CNORM_NONE && c->tune_chain_resid_d < 0 && groups <= std::max(c->cu_count, 1) && p.K / 16 > 64) {
        // [r5] the residual products with at most one row group per compute unit (llama2-7B's Wo and W2): ONE wave with a ring of 32 blocks -- no relay
        // through LDS, no barrier per chunk -- Wo 15.2 -> 13.6 us, W2 33.7 -> 32.7 (profiles/r05_experiments.md)
        W = 1; D = 32;
    }
    else {
        const int cus = std::max(c->cu_count, 1);
        if (groups >= 5 * cus) { W = 1; D = 16; }   // W1 | W3, classifier: several groups per SIMD, each with its own ring
        else { W = 2; D = 16; }                     // one to three groups per CU (tools/chain_sweep.py: 216 best or equal everywhere)
        if (p.K / 16 <= 2 * D) { W = 1; D = 16; }   // a row of a few blocks: nothing to relay
    }
    if (norm == CNORM_LEAD && c->tune_chain_lead_w > 0 && c->tune_chain_d <= 0) { W = c->tune_chain_lead_w; D = 16; }      // ("chain_lead_w": the leader launches' waves per row group)
    if ((size_t)(p.K + chain_pad_floats(W, D, 4)) * sizeof(float) > 64 * 1024) { W = 1; D = 16; }
    const size_t lds = (size_t)(p.K + chain_pad_floats(W, D, 4)) * sizeof(float);      // x + the zeros behind it
    REQUIRE(lds <= 64 * 1024, RAMA_EUNSUP, "chain-order matvec: row longer than ~15800 floats");
    // [r5] one wave per row group and more groups than compute units: the groups that do not divide by the CUs as halves (chain.hpp half_from; "chain_split")
    int nblocks = groups;
    p.half_from = 0;
    if (c->tune_chain_split && W == 1 && D == 16 && c->tune_chain_d <= 0 && norm != CNORM_EXACT && norm != CNORM_TREE) {
        const int cus = std::max(c->cu_count, 1), rem = groups % cus;
        // (more than half the CUs with a group more -- the classifier's 2 000 groups: the halves would give some CUs two again)
        if (groups > cus && rem > 0 && 2 * rem <= cus) { p.half_from = groups - rem; nblocks = groups + rem; }
    }
    const bool wo_like = EPI == CEPI_RESID && norm == CNORM_NONE && p.K == p.rows;      // the square residual product: Wo
    const dim3 grid(nblocks);
    if (norm == CNORM_LEAD) {      // the exact sum by a leader workgroup of this launch (grid + 1); geometry as without a norm
        REQUIRE(D == 16 && (W == 1 || W == 2) && p.K % 8 == 0 && p.K <= 4096 * W && (EPI == CEPI_QKV || EPI == CEPI_SWIGLU || EPI == CEPI_STORE) && p.lead && p.epoch && p.err,
                RAMA_EUNSUP, "chain-order matvec: no leader-norm instantiation for this shape");
        constexpr int E3 = (EPI == CEPI_QKV || EPI == CEPI_SWIGLU || EPI == CEPI_STORE) ? EPI : CEPI_QKV;
        const int per = (p.K + 64 * W - 1) / (64 * W);
        const size_t ldsl = std::max(lds, W == 1 ? sizeof(FastSumShared<1>) : sizeof(FastSumShared<2>));
        const dim3 gridl(nblocks + 1);
#define RAMA_CHAIN_L(W_, LR_) RAMA_LAUNCH(c, (gemv_chain_kernel<W_, 16, 4, E3, CNORM_LEAD, LR_>), gridl, dim3(W_ * 64), ldsl, p)
#define RAMA_CHAIN_LW(W_) do { if (per <= 8) RAMA_CHAIN_L(W_, 8); else if (per <= 16) RAMA_CHAIN_L(W_, 16); else if (per <= 32) RAMA_CHAIN_L(W_, 32); else RAMA_CHAIN_L(W_, 64); } while (0)
        if (W == 1) RAMA_CHAIN_LW(1); else RAMA_CHAIN_LW(2);
#undef RAMA_CHAIN_LW
#undef RAMA_CHAIN_L
        LAUNCHCHK();
        c->handoff_dirty = true;
        return 0;
    }
    if (norm != CNORM_NONE) {      // the rmsnorm folded in: all of x sits in the workgroup's registers (K <= 64 x threads)
        if (c->tune_chain_d <= 0 && W == 1 && p.K > 4096) W = 2;
        REQUIRE(chain_norm_fits(p.K, norm) && p.K <= 4096 * W && D == 16 && (W == 1 || W == 2) && EPI != CEPI_RESID, RAMA_EUNSUP, "chain-order matvec: no norm-folding instantiation for this shape");
        size_t ldsn = (size_t)(p.K + chain_pad_floats(W, D, 4)) * sizeof(float);
        if (norm == CNORM_EXACT) ldsn += ((size_t)p.K + ((size_t)p.K >> 5) + 4) * sizeof(float);      // + the squares, scan_slot layout
        constexpr int E = EPI != CEPI_RESID ? EPI : CEPI_QKV;
#define RAMA_CHAIN_N(W_, N_) RAMA_LAUNCH(c, (gemv_chain_kernel<W_, 16, 4, E, N_>), grid, dim3(W_ * 64), ldsn, p)
        if (norm == CNORM_TREE) { if (W == 1) RAMA_CHAIN_N(1, CNORM_TREE); else RAMA_CHAIN_N(2, CNORM_TREE); }
        else {
            REQUIRE(EPI == CEPI_QKV || EPI == CEPI_SWIGLU, RAMA_EUNSUP, "chain-order matvec: the lane-ripple norm folds into Wq|Wk|Wv and W1|W3 only");
            constexpr int E2 = (EPI == CEPI_QKV || EPI == CEPI_SWIGLU) ? EPI : CEPI_QKV;
            if (W == 1) RAMA_LAUNCH(c, (gemv_chain_kernel<1, 16, 4, E2, CNORM_EXACT>), grid, dim3(64), ldsn, p);
            else RAMA_LAUNCH(c, (gemv_chain_kernel<2, 16, 4, E2, CNORM_EXACT>), grid, dim3(128), ldsn, p);
        }
#undef RAMA_CHAIN_N
        LAUNCHCHK();
        return 0;
    }
#define RAMA_CHAIN(W_, D_) RAMA_LAUNCH(c, (gemv_chain_kernel<W_, D_, 4, EPI>), grid, dim3(W_ * 64), lds, p)
    if (W == 1 && D == 16) RAMA_CHAIN(1, 16);
    else if (W == 1 && D == 32 && wo_like) RAMA_LAUNCH(c, (gemv_chain_kernel<1, 32, 4, EPI, CNORM_NONE, 64, 1>), grid, dim3(64), lds, p);      // (Wo under a name of its own)
    else if (W == 1 && D == 32) RAMA_CHAIN(1, 32);
    else if (W == 2 && D == 16) RAMA_CHAIN(2, 16);
    else if (W == 2 && D == 32) RAMA_CHAIN(2, 32);

    else if (W == 4 && D == 16) RAMA_CHAIN(4, 16);
    else if (W == 4 && D == 32) RAMA_CHAIN(4, 32);
    else return fail(RAMA_EINVAL, "chain-order matvec: no such geometry", __FILE__, __LINE__);
#undef RAMA_CHAIN
    LAUNCHCHK();
    return 0;
}
// the entry the other translation units call: the epilogue as an argument.  The (epilogue, norm) pairs are those some caller uses -- the
// residual products fold no norm, the plain store none by lane ripples --, which keeps the instantiated kernels to exactly these four templates'
int launch_chain(rama_ctx* c, ChainParams& p, int epi, int norm) {
    switch (epi) {
        case CEPI_STORE: if (norm == CNORM_EXACT) break; return launch_chain_epi<CEPI_STORE>(c, p, norm);
        case CEPI_RESID: if (norm != CNORM_NONE) break; return launch_chain_epi<CEPI_RESID>(c, p, norm);
        case CEPI_QKV: return launch_chain_epi<CEPI_QKV>(c, p, norm);
        case CEPI_SWIGLU: return launch_chain_epi<CEPI_SWIGLU>(c, p, norm);
    }
    return fail(RAMA_EINVAL, "chain-order matvec: no launch for this epilogue and norm", __FILE__, __LINE__);
}
bool rmsnorm_chain_ok(size_t n) { return n <= (size_t)kNormMax && (n + (n >> 5) + 2) * sizeof(float) <= 64 * 1024; }
int launch_rmsnorm_chain(rama_ctx* c, float* o, const float* x, const float* w, int n, float* copy_to, int batch, int stride, const SeqSlot* tile) {
    const size_t lds = ((size_t)n + ((size_t)n >> 5) + 2) * sizeof(float);
    RAMA_LAUNCH(c, rmsnorm_chain_kernel, dim3(batch), dim3(kNormThreads), lds, o, x, w, n, copy_to, stride, tile);
    LAUNCHCHK();
    return 0;
}
int launch_softmax_chain(rama_ctx* c, float* x, int n) {      // n: rmsnorm_chain_ok
    hipLaunchKernelGGL(softmax_chain_kernel, dim3(1), dim3(kNormThreads), ((size_t)n + ((size_t)n >> 5) + 2) * sizeof(float), c->stream, x, n);
    LAUNCHCHK();
    return 0;
}
size_t attn_chain_lds_bytes(int head_size, int seq_len, int nw) { return attn_chain_lds_floats(head_size, seq_len, nw) * sizeof(float) + 16; }
int attn_chain_waves(int head_size, bool long_ctx) {
    const int want = long_ctx ? 8 : 4;
    return attn_chain_fits(head_size, want) ? want : (attn_chain_fits(head_size, 8) ? 8 : 16);
}
bool attn_chain_ok(int head_size, int seq_len) {      // the largest variant a launch may pick must fit
    if (head_size % 4 || !attn_chain_fits(head_size, 16)) return false;
    return attn_chain_lds_bytes(head_size, seq_len, attn_chain_waves(head_size, true)) <= kAttnChainMaxLds;
}
// the score scratch of parity mode's spread attention; inside a stream capture nothing is allocated (the caller then keeps
// the three-launch form, whose softmax rewrites each head's row from ONE workgroup)
int ensure_attn_scores(rama_ctx* c, int n_heads, int seq_len) {
    const size_t need = (size_t)n_heads * (size_t)seq_len;
    if (need <= c->attn_scores_floats) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return 0; }
    if (c->attn_scores) { HIPCHK(hipStreamSynchronize(c->stream)); drop_graph(c); HIPCHK(hipFree(c->attn_scores)); c->attn_scores = nullptr; c->attn_scores_floats = 0; }      // (graphs captured for a smaller model hold the old address)
    HIPCHK(hipMalloc(&c->attn_scores, need * sizeof(float)));
    c->attn_scores_floats = need;
    return 0;
}

// long_ctx: 8 waves per head (twice the timesteps per score round, twice the loaders of the value tiles) -- from position 256 on
int launch_attention_chain(rama_ctx* c, float* xb, float* att, const float* q, const float* kc_layer, const float* vc_layer,
                                  const Ctl* ctl, int pos, int dim, int head_size, int seq_len, int n_heads, bool long_ctx, bool spread_wanted) {
    // spread: the three-launch form for long contexts; it needs whole staged pieces and 32-column slices, a score
    // buffer that fits the softmax kernel's LDS, and the att buffer
    const bool spread = spread_wanted && att && head_size % kAttPiece == 0 && head_size % kValCols == 0 && head_size <= 256 &&
                        ((size_t)seq_len + ((size_t)seq_len >> 5) + 4) * sizeof(float) <= 60 * 1024;
    REQUIRE(aligned16(q) && aligned16(kc_layer) && aligned16(vc_layer) && dim % 4 == 0, RAMA_EINVAL, "attention: buffers must be 16-byte aligned");
    RefAttnParams p{};
    p.q = q; p.kc = kc_layer; p.vc = vc_layer; p.att = att; p.xb = xb; p.ctl = ctl; p.pos_val = pos;
    p.dim = dim; p.head_size = head_size; p.seq_len = seq_len;
    if (spread) {
        // two launches over the whole chip (chain.hpp; three with "attn_fv" = 0): needs att (the scores / probabilities travel through it)
        // (an armed kernel-class timer brackets the whole attention: its start event rides on the first launch, its stop event on the last)
        const int ngroups = (seq_len + 63) / 64;
        // the one-launch softmax + values form reads the scores in every (head, slice) workgroup while the slice-0 workgroup of the head writes
        // the probabilities: the scores therefore travel through a scratch of their own, never through the buffer that receives the probabilities
        const size_t fv_lds = attn_fused_values_lds_floats(seq_len) * sizeof(float);
        bool fv = c->tune_attn_fv && fv_lds <= 32 * 1024;
        if (fv) {
            const int rs = ensure_attn_scores(c, n_heads, seq_len); if (rs) return rs;
            fv = c->attn_scores_floats >= (size_t)n_heads * (size_t)seq_len;
        }
        p.sc = fv ? c->attn_scores : att;
        hipEvent_t ev_start = c->cur_start, ev_stop = c->cur_start ? c->cur_stop : nullptr;
        c->cur_start = nullptr;
        if (ev_start) hipExtLaunchKernelGGL(attn_scores_chain_kernel, dim3(n_heads, ngroups), dim3(64), 0, c->stream, ev_start, nullptr, 0, p);
        else hipLaunchKernelGGL(attn_scores_chain_kernel, dim3(n_heads, ngroups), dim3(64), 0, c->stream, p);
        LAUNCHCHK();
        if (fv) {             // the softmax repeated by every slice workgroup, one launch (chain.hpp [r4])
            if (ev_stop) hipExtLaunchKernelGGL(attn_softmax_values_chain_kernel, dim3(n_heads, head_size / kValCols), dim3(kFvSoftWaves * 64), fv_lds, c->stream, nullptr, ev_stop, 0, p);
            else hipLaunchKernelGGL(attn_softmax_values_chain_kernel, dim3(n_heads, head_size / kValCols), dim3(kFvSoftWaves * 64), fv_lds, c->stream, p);
            LAUNCHCHK();
            return 0;
        }
        hipLaunchKernelGGL(attn_softmax_chain_kernel, dim3(n_heads), dim3(kSoftWaves * 64), ((size_t)seq_len + ((size_t)seq_len >> 5) + 4) * sizeof(float), c->stream, p);
        LAUNCHCHK();
        if (ev_stop) hipExtLaunchKernelGGL(attn_values_chain_kernel, dim3(n_heads, head_size / kValCols), dim3(kValWaves * 64), 0, c->stream, nullptr, ev_stop, 0, p);
        else hipLaunchKernelGGL(attn_values_chain_kernel, dim3(n_heads, head_size / kValCols), dim3(kValWaves * 64), 0, c->stream, p);
        LAUNCHCHK();
        return 0;
    }
    const int nw = attn_chain_waves(head_size, long_ctx);
    const size_t lds = attn_chain_lds_bytes(head_size, seq_len, nw);
    REQUIRE(lds <= kAttnChainMaxLds, RAMA_EUNSUP, "attention (parity mode): context too long for the score buffer");
#define RAMA_ATTN_CHAIN(NW_) RAMA_LAUNCH(c, (attention_chain_kernel<NW_>), dim3(n_heads), dim3(NW_ * 64), lds, p)
    if (nw == 4) RAMA_ATTN_CHAIN(4);
    else if (nw == 8) RAMA_ATTN_CHAIN(8);
    else RAMA_ATTN_CHAIN(16);
#undef RAMA_ATTN_CHAIN
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------- token batches in the reference's order (chain.hpp gemm_chain_kernel)

template <int EPI>
static int launch_gemm_chain_epi(rama_ctx* c, GemmChainParams& p) {
    p.lane_reduce = c->tune_lane_reduce;
    const dim3 grid(p.nmat * ((p.rows + 15) / 16)), block(kGcThreads);
    if (p.n_tok <= 4) hipLaunchKernelGGL((gemm_chain_kernel<1, EPI>), grid, block, gemm_chain_lds_bytes(1), c->stream, p);
    else if (p.n_tok <= 8) hipLaunchKernelGGL((gemm_chain_kernel<2, EPI>), grid, block, gemm_chain_lds_bytes(2), c->stream, p);
    else if (p.n_tok <= 16) hipLaunchKernelGGL((gemm_chain_kernel<4, EPI>), grid, block, gemm_chain_lds_bytes(4), c->stream, p);
    else hipLaunchKernelGGL((gemm_chain_kernel<8, EPI>), grid, block, gemm_chain_lds_bytes(8), c->stream, p);
    LAUNCHCHK();
    return 0;
}
int launch_gemm_chain(rama_ctx* c, GemmChainParams& p, int epi) {
    switch (epi) {
        case CEPI_STORE: return launch_gemm_chain_epi<CEPI_STORE>(c, p);
        case CEPI_RESID: return launch_gemm_chain_epi<CEPI_RESID>(c, p);
        case CEPI_QKV: return launch_gemm_chain_epi<CEPI_QKV>(c, p);
        case CEPI_SWIGLU: return launch_gemm_chain_epi<CEPI_SWIGLU>(c, p);
    }
    return fail(RAMA_EINVAL, "chain-order token batch: no such epilogue", __FILE__, __LINE__);
}

// parity mode's exact attention for a token batch: one workgroup of nw waves per (head, token) -- the RefAttnParams carry
// tok_stride / att_stride and either p.pos_val + token or the sequence table
int launch_attention_chain_tokens(rama_ctx* c, const RefAttnParams& a, int n_heads, int nt, int nw, size_t lds) {
    const dim3 grid(n_heads, nt);
    if (nw == 4) hipLaunchKernelGGL((attention_chain_kernel<4>), grid, dim3(4 * 64), lds, c->stream, a);
    else if (nw == 8) hipLaunchKernelGGL((attention_chain_kernel<8>), grid, dim3(8 * 64), lds, c->stream, a);
    else hipLaunchKernelGGL((attention_chain_kernel<16>), grid, dim3(16 * 64), lds, c->stream, a);
    LAUNCHCHK();
    return 0;
}

// the same grid for the rows of a tree pass (q8_tree.hpp): a timestep behind the root's position is read from an ancestor's row of the pass
// (by_node: a level of a draft model's tree, q8_spec_model_tree.hpp -- a.kr / a.v are the layer's slice of the draft tree store, the path's nibbles nodes)
int launch_attention_tree(rama_ctx* c, const TreeAttnParams& a, int n_heads, int nt, int nw, size_t lds, bool by_node) {
    const dim3 grid(n_heads, nt);
    if (by_node) {
        if (nw == 4) hipLaunchKernelGGL((attention_draft_tree_kernel<4>), grid, dim3(4 * 64), lds, c->stream, a);
        else if (nw == 8) hipLaunchKernelGGL((attention_draft_tree_kernel<8>), grid, dim3(8 * 64), lds, c->stream, a);
        else hipLaunchKernelGGL((attention_draft_tree_kernel<16>), grid, dim3(16 * 64), lds, c->stream, a);
        LAUNCHCHK();
        return 0;
    }
    if (nw == 4) hipLaunchKernelGGL((attention_tree_kernel<4>), grid, dim3(4 * 64), lds, c->stream, a);
    else if (nw == 8) hipLaunchKernelGGL((attention_tree_kernel<8>), grid, dim3(8 * 64), lds, c->stream, a);
    else hipLaunchKernelGGL((attention_tree_kernel<16>), grid, dim3(16 * 64), lds, c->stream, a);
    LAUNCHCHK();
    return 0;
}

// ---- device top-p sampler (topp_sort.hpp: block sorts + ranks + the exact running sum; every kernel hand-written)

// topp_pick_dist_kernel's hand-off words in one allocation: items | hdr | cross | epoch | bad
constexpr size_t kToppDistItems = sizeof(PickItem) * kPickChunk * kPickMaxChunks;
constexpr size_t kToppDistBytes = kToppDistItems + 8 * kPickMaxChunks + 16 + 16;
static ToppDistParams topp_dist_params(rama_ctx* c) {
    char* b = (char*)c->topp_dist;
    ToppDistParams d{};
    d.approx = c->topp_approx;
    d.items = (PickItem*)b;
    d.hdr = (unsigned long long*)(b + kToppDistItems);
    d.cross = d.hdr + kPickMaxChunks;
    d.epoch = (const unsigned*)(d.cross + 2);
    d.bad = (unsigned*)(d.cross + 2) + 1;
    return d;
}
// The error word of the distributed top-p pick (topp_pick.hpp ToppDistParams::bad; bit 0: a bounded wait gave up -- the launch then drained without
// ending the step: no token, the cursor not advanced; bit 1: a predicted binade did not hold -- the token came from wrong sums) is read at every
// synchronising exit like the hand-off word above: the call fails and the word is cleared, so that one hiccup neither leaves with rc 0 nor
// makes every later launch give up its waits after 1 024 spins (bit 0 is what the waiting workgroups watch).  The stream is idle when this runs.
int topp_dist_check(rama_ctx* c) {
    if (!c->topp_dist || !c->topp_dist_dirty) return 0;      // (gated like handoff_dirty: no device round trip per rama_sync of a host-driven loop)
    c->topp_dist_dirty = false;
    unsigned bad = 0;
    unsigned* word = topp_dist_params(c).bad;
    HIPCHK(hipMemcpy(&bad, word, sizeof bad, hipMemcpyDeviceToHost));
    if (!bad) return 0;
    HIPCHK(hipMemset(word, 0, sizeof bad));
    return fail(RAMA_EINVAL, (bad & 1u) ? "top-p sampler: a hand-off of the distributed pick timed out (no token was produced)"
                                        : "top-p sampler: a predicted binade of the running sum did not hold (the token is not trustworthy)", __FILE__, __LINE__);
}
// test entry (not in the C ABI header): set the word, as a launch whose wait gave up would
extern "C" int rama_internal_topp_dist_poke(rama_ctx* c, unsigned value) {
    RAMA_ENTER(c);
    if (!c || !c->topp_dist) return 1;
    hipStreamSynchronize(c->stream);
    c->topp_dist_dirty = true;
    return hipMemcpy(topp_dist_params(c).bad, &value, sizeof value, hipMemcpyHostToDevice) != hipSuccess;
}
// diagnostics (not in the C ABI header): bit 0 a hand-off wait of topp_pick_dist_kernel timed out, bit 1 a predicted binade did not hold
extern "C" int rama_internal_topp_dist_bad(rama_ctx* c, unsigned* bad) {
    RAMA_ENTER(c);
    if (!c || !bad) return 1;
    *bad = 0;
    if (!c->topp_dist) return 0;
    hipStreamSynchronize(c->stream);
    return hipMemcpy(bad, topp_dist_params(c).bad, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess;
}

// scratch for n logits; called outside any stream capture
int ensure_topp_scratch(rama_ctx* c, int n) {
    if (n <= c->topp_cap) return 0;
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t nblk = ((size_t)n + kToppBlock - 1) / kToppBlock;
    hipFree(c->topp_keys[1]); hipFree(c->topp_vals[1]);
    HIPCHK(hipMalloc(&c->topp_keys[1], sizeof(float) * n));
    HIPCHK(hipMalloc(&c->topp_vals[1], sizeof(int) * n));
    hipFree(c->topp_prefix); HIPCHK(hipMalloc(&c->topp_prefix, sizeof(float) * n));
    if (!c->topp_m) { HIPCHK(hipMalloc(&c->topp_m, sizeof(int))); HIPCHK(hipMalloc(&c->topp_err, sizeof(unsigned))); HIPCHK(hipMemset(c->topp_err, 0, sizeof(unsigned))); }
    hipFree(c->topp_bp); hipFree(c->topp_bi); hipFree(c->topp_bcount); hipFree(c->topp_racc);
    HIPCHK(hipMalloc(&c->topp_racc, sizeof(int) * kToppBlock * std::max<size_t>(nblk, kToppMaxBlocks)));
    HIPCHK(hipMalloc(&c->topp_bp, sizeof(float) * kToppBlock * std::max<size_t>(nblk, kToppMaxBlocks)));
    HIPCHK(hipMalloc(&c->topp_bi, sizeof(int) * kToppBlock * std::max<size_t>(nblk, kToppMaxBlocks)));
    HIPCHK(hipMalloc(&c->topp_bcount, sizeof(int) * std::max<size_t>(((size_t)n + 511) / 512 + 1, std::max<size_t>(nblk, kToppMaxBlocks))));
    hipFree(c->topp_stats); HIPCHK(hipMalloc(&c->topp_stats, sizeof(ToppStats) * (((size_t)n + 1023) / 1024 + 1)));
    hipFree(c->topp_rk); hipFree(c->topp_bm); hipFree(c->topp_approx);
    HIPCHK(hipMalloc(&c->topp_rk, sizeof(unsigned long long) * kToppBlock * std::max<size_t>(nblk, kToppMaxBlocks)));
    HIPCHK(hipMalloc(&c->topp_bm, sizeof(unsigned long long) * kToppBlock * std::max<size_t>(nblk, kToppMaxBlocks)));
    HIPCHK(hipMalloc(&c->topp_approx, sizeof(float) * n));
    if (!c->topp_dist) { HIPCHK(hipMalloc(&c->topp_dist, kToppDistBytes)); HIPCHK(hipMemset(c->topp_dist, 0, kToppDistBytes)); }
    c->topp_cap = n;
    return 0;
}

// [r4] the small-block ordering: partial statistics, BS-entry block sorts, (block, OB blocks) pair ranking, scatter
template <int BS, int OB>
static int enqueue_small_blocks(rama_ctx* c, ToppSortParams sp, int nstat) {
    sp.nblk = (sp.n + BS - 1) / BS;
    hipLaunchKernelGGL(topp_stats_kernel, dim3(nstat), dim3(1024), 0, c->stream, sp, c->topp_stats);
    LAUNCHCHK();
    hipLaunchKernelGGL(topp_blocksort_bs_kernel<BS>, dim3(sp.nblk), dim3(BS), 0, c->stream, sp, (const ToppStats*)c->topp_stats, nstat);
    LAUNCHCHK();
    hipLaunchKernelGGL((topp_rank_pairs_bs_kernel<BS, OB>), dim3(sp.nblk, (sp.nblk + OB - 1) / OB), dim3(BS / 2), 0, c->stream, sp);
    LAUNCHCHK();
    hipLaunchKernelGGL(topp_rank_scatter_bs_kernel<BS>, dim3((sp.nblk * BS + 1023) / 1024), dim3(1024), 0, c->stream, sp);
    LAUNCHCHK();
    return 0;
}

static int enqueue_sample_launches(rama_ctx* c, ArgmaxParams fin, float temperature, float topp, float u) {
    if (temperature == 0.0f) {
        hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, c->stream, fin);
        LAUNCHCHK();
        return 0;
    }
    REQUIRE(fin.n > 1 && fin.n <= c->topp_cap, RAMA_EINVAL, "top-p sampler: scratch not prepared");
    ToppParams tp{};
    tp.logits = fin.logits; tp.n = fin.n; tp.temperature = temperature; tp.topp = topp; tp.u = u;
    tp.keys = c->topp_keys[1]; tp.vals = c->topp_vals[1]; tp.prefix = c->topp_prefix; tp.m = c->topp_m; tp.err = c->topp_err;
    // block sorts in LDS, then every kept entry's rank by binary searches in the other blocks (topp_sort.hpp): through LDS
    // when the whole list fits one workgroup's LDS (n <= 32768), through global memory otherwise (or with "topp_sort" = 0)
    const bool lds_path = c->tune_topp_sort && fin.n <= kToppBlock * kToppMaxBlocks;
    ToppSortParams sp{};
    sp.logits = fin.logits; sp.n = fin.n; sp.temperature = temperature; sp.topp = topp;
    sp.bp = c->topp_bp; sp.bi = c->topp_bi; sp.bcount = c->topp_bcount; sp.keys = c->topp_keys[1]; sp.vals = c->topp_vals[1];
    sp.m = c->topp_m; sp.err = c->topp_err; sp.nblk = (fin.n + kToppBlock - 1) / kToppBlock;
    const bool pairs = lds_path && c->tune_topp_pairs && sp.nblk > 1;
    if (pairs) sp.racc = c->topp_racc;
    bool dist = false;
    if (pairs && c->tune_topp_block != kToppBlock) {
        sp.rk = c->topp_rk; sp.bm = c->topp_bm; sp.approx = c->topp_approx;
        dist = c->tune_topp_dist != 0;
        if (dist) sp.epoch = (unsigned*)topp_dist_params(c).epoch;
        // small blocks (topp_sort.hpp [r4]): the statistics once per 1024 logits, 1024-entry sorts on 8 waves (or 512 on 4), the ranking by
        // (block, block) pairs over the whole chip, a scatter launch
        const int nstat = (fin.n + 1023) / 1024;
        if (c->tune_topp_block == 1024) { if (int rc = enqueue_small_blocks<1024, 2>(c, sp, nstat)) return rc; }
        else if (int rc = enqueue_small_blocks<512, 4>(c, sp, nstat)) return rc;
    } else {
    if (fin.n <= kToppBlock * kToppMaxBlocks) hipLaunchKernelGGL(topp_blocksort_kernel<false>, dim3(sp.nblk), dim3(1024), 0, c->stream, sp);
    else hipLaunchKernelGGL(topp_blocksort_kernel<true>, dim3(sp.nblk), dim3(1024), 0, c->stream, sp);
    LAUNCHCHK();
    if (pairs) {
        hipLaunchKernelGGL(topp_rank_pairs_kernel, dim3(sp.nblk, sp.nblk), dim3(1024), 0, c->stream, sp);
        LAUNCHCHK();
        hipLaunchKernelGGL(topp_rank_scatter_kernel, dim3(sp.nblk * (kToppBlock / 1024)), dim3(1024), 0, c->stream, sp);
    } else if (lds_path) hipLaunchKernelGGL(topp_rank_kernel<kToppMaxBlocks>, dim3(sp.nblk * (kToppBlock / kRankThreads)), dim3(kRankThreads), 0, c->stream, sp);
    else hipLaunchKernelGGL(topp_rank_global_kernel, dim3(sp.nblk * (kToppBlock / 256)), dim3(256), 0, c->stream, sp);
    LAUNCHCHK();
    }
    if (lds_path && !c->tune_topp_keep_sums) tp.prefix = nullptr;
    // the running sums: the exact parallel scan with the list in LDS, or (longer lists) the staged lane ripple
    if (dist) { c->topp_dist_dirty = true; hipLaunchKernelGGL(topp_pick_dist_kernel, dim3(kPickMaxChunks), dim3(1024), 0, c->stream, tp, topp_dist_params(c), fin); }
    else if (lds_path) hipLaunchKernelGGL(topp_pick_scan_kernel, dim3(1), dim3(1024), 0, c->stream, tp, fin);
    else hipLaunchKernelGGL(topp_pick_kernel, dim3(1), dim3(1024), 0, c->stream, tp, fin);
    LAUNCHCHK();
    return 0;
}
// the sampling tail of a step: argmax (temperature 0) or top-p, then whatever `fin` asks for
// (result word, cursor advance, next embedding gather)
int enqueue_sample(rama_ctx* c, ArgmaxParams fin, float temperature, float topp, float u) {
    // kernel class RAMA_K_SAMPLE: up to five launches, so the bracket is a pair of event records around them (eager mode only)
    KProf& k = c->kp;
    const bool timed = k.kernel_id == RAMA_K_SAMPLE && k.used < k.max_records;
    if (timed) HIPCHK(hipEventRecord(k.ev[2 * k.used], c->stream));
    const int rc = enqueue_sample_launches(c, fin, temperature, topp, u);
    if (timed) { HIPCHK(hipEventRecord(k.ev[2 * k.used + 1], c->stream)); k.used++; }
    return rc;
}

int rama_sample_topp_dev(rama_ctx* c, const float* logits, size_t n, float temperature, float topp, float u, int32_t* result_dev) {
    RAMA_ENTER(c);
    REQUIRE(c && logits && result_dev && n > 1 && n < (1u << 30), RAMA_EINVAL, "sample_topp_dev: bad argument");
    int rc = temperature != 0.0f ? ensure_topp_scratch(c, (int)n) : 0;
    if (rc) return rc;
    ArgmaxParams ap{};
    ap.logits = logits; ap.n = (int)n; ap.result = (int*)result_dev;
    return enqueue_sample(c, ap, temperature, topp, u);
}

// ---- the batched top-p sampler: many rows per launch (topp_sort.hpp ROWS kernels), the parallelism from the rows -- no waits between
// workgroups (topp_pick_dist_kernel's hand-offs need all its workgroups resident: not at 128 rows), the pick one workgroup per row
bool topp_params_ok(float temperature, float topp, float u) {
    return temperature >= 0.0f && topp >= 0.0f && topp <= 1.0f && u >= 0.0f && u < 1.0f;      // (false for NaN)
}
// slices for `rows` rows of n <= 32768 logits; called outside any stream capture
int ensure_topp_batch(rama_ctx* c, int rows, int n) {
    auto& t = c->tb;
    size_t rs = ((size_t)n + kToppBlock - 1) / kToppBlock * kToppBlock;      // >= n and >= the blocks' slots of either block size
    if (rows <= t.rows && rs <= t.rstride) return 0;
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    drop_graph(c);                                                 // a captured chained step holds the old slices
    rows = std::max(rows, t.rows); rs = std::max(rs, t.rstride);
    for (void** q : {(void**)&t.keys, (void**)&t.vals, (void**)&t.bp, (void**)&t.bi, (void**)&t.rk, (void**)&t.bm, (void**)&t.bcount, (void**)&t.stats, (void**)&t.m}) {
        hipFree(*q); *q = nullptr;
    }
    t.rows = 0; t.rstride = 0;
    const size_t e = (size_t)rows * rs;
    HIPCHK(hipMalloc(&t.keys, sizeof(float) * e)); HIPCHK(hipMalloc(&t.vals, sizeof(int) * e));
    HIPCHK(hipMalloc(&t.bp, sizeof(float) * e)); HIPCHK(hipMalloc(&t.bi, sizeof(int) * e));
    HIPCHK(hipMalloc(&t.rk, sizeof(unsigned long long) * e)); HIPCHK(hipMalloc(&t.bm, sizeof(unsigned long long) * e));
    HIPCHK(hipMalloc(&t.bcount, sizeof(int) * rows * kToppRowBlocks)); HIPCHK(hipMalloc(&t.stats, sizeof(ToppStats) * rows * kToppRowBlocks));
    HIPCHK(hipMalloc(&t.m, sizeof(int) * rows));
    if (!t.rows_dev) HIPCHK(hipMalloc(&t.rows_dev, sizeof(ToppRow) * kMfMaxTok));
    t.rows = rows; t.rstride = rs;
    return 0;
}
// every row's (T, topp, u) by value: the launch takes a copy, so no host staging buffer has to outlive the call
struct ToppRowsArg { float temperature[kMfMaxTok], topp[kMfMaxTok], u[kMfMaxTok]; };
__global__ void topp_rows_kernel(ToppRowsArg a, ToppRow* rows, int n_rows) {
    const int r = threadIdx.x;
    if (r < n_rows) rows[r] = ToppRow{a.temperature[r], a.topp[r], a.u[r], 0, nullptr};
}
// the sampler over n_rows rows of n <= 32768 logits (row r at logits + r ld); fin says where the picks go.  The statistics, the block
// sorts and the ranking are the single-row sampler's launches for the same n (enqueue_sample_launches at the default tuning), so every
// sampled row gets its bits; the running sums are topp_pick_scan_kernel's, one workgroup per row.
// (its ordering launches -- everything but the pick -- are enqueue_topp_batch_order: the serving chain ends its step in a pick of its own)
int enqueue_topp_batch_order(rama_ctx* c, const ToppRow* rows, int n_rows, const float* logits, size_t ld, int n, const SeqSlot* seqs) {
    auto& t = c->tb;
    REQUIRE(n > 1 && n <= kToppBlock * kToppMaxBlocks && n_rows <= t.rows && (size_t)n <= t.rstride, RAMA_EINVAL, "top-p batch sampler: scratch not prepared");
    ToppSortParams sp{};
    sp.logits = logits; sp.n = n;
    sp.bp = t.bp; sp.bi = t.bi; sp.bcount = t.bcount; sp.keys = t.keys; sp.vals = t.vals; sp.m = t.m;
    sp.rows = rows; sp.seqs = seqs; sp.ld = ld; sp.rstride = t.rstride;
    if (n <= kToppBlock) {                                         // one block: its own statistics and sort, the in-LDS ranking
        sp.nblk = 1;
        hipLaunchKernelGGL((topp_blocksort_kernel<false, true>), dim3(1, 1, n_rows), dim3(1024), 0, c->stream, sp);
        LAUNCHCHK();
        hipLaunchKernelGGL((topp_rank_kernel<kToppMaxBlocks, true>), dim3(kToppBlock / kRankThreads, 1, n_rows), dim3(kRankThreads), 0, c->stream, sp);
        LAUNCHCHK();
    } else {                                                       // the small-block path: statistics per 1024 logits, 1024-entry sorts, pairs, scatter
        // (pair width OB = 2 as the single-row path: 4 and 8 -- fewer atomics, wider workgroups -- measured 3 % and 44 % slower at 128 rows)
        constexpr int BS = 1024, OB = 2;
        sp.rk = t.rk; sp.bm = t.bm;
        sp.nblk = (n + BS - 1) / BS;
        const int nstat = (n + 1023) / 1024;
        hipLaunchKernelGGL(topp_stats_kernel<true>, dim3(nstat, 1, n_rows), dim3(1024), 0, c->stream, sp, t.stats);
        LAUNCHCHK();
        hipLaunchKernelGGL((topp_blocksort_bs_kernel<BS, true>), dim3(sp.nblk, 1, n_rows), dim3(BS), 0, c->stream, sp, (const ToppStats*)t.stats, nstat);
        LAUNCHCHK();
        hipLaunchKernelGGL((topp_rank_pairs_bs_kernel<BS, OB, true>), dim3(sp.nblk, (sp.nblk + OB - 1) / OB, n_rows), dim3(BS / 2), 0, c->stream, sp);
        LAUNCHCHK();
        hipLaunchKernelGGL((topp_rank_scatter_bs_kernel<BS, true>), dim3((sp.nblk * BS + 1023) / 1024, 1, n_rows), dim3(1024), 0, c->stream, sp);
        LAUNCHCHK();
    }
    return 0;
}
int enqueue_topp_batch(rama_ctx* c, const ToppRow* rows, int n_rows, const float* logits, size_t ld, int n, ToppBatchParams fin) {
    auto& t = c->tb;
    { const int rc = enqueue_topp_batch_order(c, rows, n_rows, logits, ld, n, fin.seqs); if (rc) return rc; }
    fin.rows = rows; fin.logits = logits; fin.ld = ld; fin.n = n;
    fin.keys = t.keys; fin.vals = t.vals; fin.m = t.m; fin.rstride = t.rstride;
    hipLaunchKernelGGL(topp_pick_batch_kernel, dim3(n_rows), dim3(1024), 0, c->stream, fin);
    LAUNCHCHK();
    return 0;
}

int rama_sample_topp_batch_dev(rama_ctx* c, const float* logits, size_t ld, size_t n, int n_rows, const float* temperature_host,
                               const float* topp_host, const float* u_host, int32_t* result_dev) {
    RAMA_ENTER(c);
    REQUIRE(c && logits && temperature_host && topp_host && u_host && result_dev, RAMA_EINVAL, "sample_topp_batch_dev: NULL argument");
    REQUIRE(n > 1 && n < (1u << 30) && ld >= n && n_rows >= 1 && n_rows <= kMfMaxTok, RAMA_EINVAL, "sample_topp_batch_dev: 1..128 rows of n > 1 logits, ld >= n");
    for (int r = 0; r < n_rows; r++)
        REQUIRE(topp_params_ok(temperature_host[r], topp_host[r], u_host[r]), RAMA_EINVAL, "sample_topp_batch_dev: temperature >= 0, topp in [0,1], u in [0,1)");
    if (set_device(c)) return 1;
    if (n > (size_t)kToppBlock * kToppMaxBlocks) {
        // beyond one workgroup's LDS the single-row sampler ranks through global memory and picks with a staged ripple: row by row
        for (int r = 0; r < n_rows; r++) {
            if (temperature_host[r] != 0.0f) { int rc = ensure_topp_scratch(c, (int)n); if (rc) return rc; }
            ArgmaxParams ap{};
            ap.logits = logits + (size_t)r * ld; ap.n = (int)n; ap.result = (int*)result_dev + r;
            int rc = enqueue_sample_launches(c, ap, temperature_host[r], topp_host[r], u_host[r]); if (rc) return rc;
        }
        return 0;
    }
    int rc = ensure_topp_batch(c, n_rows, (int)n); if (rc) return rc;
    ToppRowsArg a{};
    for (int r = 0; r < n_rows; r++) { a.temperature[r] = temperature_host[r]; a.topp[r] = topp_host[r]; a.u[r] = u_host[r]; }
    hipLaunchKernelGGL(topp_rows_kernel, dim3(1), dim3(kMfMaxTok), 0, c->stream, a, c->tb.rows_dev, n_rows);
    LAUNCHCHK();
    ToppBatchParams fin{};
    fin.result = (int*)result_dev;
    return enqueue_topp_batch(c, c->tb.rows_dev, n_rows, logits, ld, (int)n, fin);
}

int rama_decode_sampler(rama_ctx* c, float temperature, float topp, float u) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    REQUIRE(topp_params_ok(temperature, topp, u), RAMA_EINVAL, "decode_sampler: temperature >= 0, topp in [0,1], u in [0,1)");
    if (temperature != c->samp_T || topp != c->samp_topp || u != c->samp_u) {
        HIPCHK(hipStreamSynchronize(c->stream));
        drop_graph(c);
        c->samp_T = temperature; c->samp_topp = topp; c->samp_u = u;
    }
    return 0;
}

int rama_argmax_dev(rama_ctx* c, const float* logits, size_t n, int32_t* result_dev) {
    RAMA_ENTER(c);
    REQUIRE(c && logits && result_dev && n > 0, RAMA_EINVAL, "argmax_dev: bad argument");
    ArgmaxParams ap{};
    ap.logits = logits; ap.n = (int)n; ap.result = (int*)result_dev;
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, c->stream, ap);
    LAUNCHCHK();
    return 0;
}

int rama_sample_argmax(rama_ctx* c, const float* logits, size_t n, int32_t* next_host) {
    RAMA_ENTER(c);
    REQUIRE(c && logits && next_host && n > 0, RAMA_EINVAL, "sample_argmax: bad argument");
    ArgmaxParams ap{};
    ap.logits = logits; ap.n = (int)n; ap.result = c->argmax_result;
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, c->stream, ap);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(c->pinned_int, c->argmax_result, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *next_host = c->pinned_int[0];
    return 0;
}

int rama_sample_topp(rama_ctx* c, const float* logits, size_t n, float temperature, float topp, float u, int32_t* next_host) {
    RAMA_ENTER(c);
    REQUIRE(c && logits && next_host && n > 1, RAMA_EINVAL, "sample_topp: bad argument");
    if (temperature == 0.0f) return rama_sample_argmax(c, logits, n, next_host);
    // Device::sample (cpu.rs:168-178) on the device; only the 4-byte result crosses PCIe (the
    // reference's GPU path downloads all n logits and samples on the host, gpu.rs:149-173)
    int rc = rama_sample_topp_dev(c, logits, n, temperature, topp, u, c->argmax_result);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->pinned_int, c->argmax_result, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hipMemsetAsync(c->topp_err, 0, sizeof(unsigned), c->stream);
    REQUIRE(c->pinned_int[0] >= 0, RAMA_EINVAL, "sample_topp: no candidate above the cutoff (the reference underflows here)");
    *next_host = c->pinned_int[0];
    return 0;
}
