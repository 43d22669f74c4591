// rama_api.hip -- the C ABI of include/rama_hip.h: context, memory, the 1:1 Device<T>
// ops, the fused decode path, the chained decode and generate, the tuning table, measurement.  Kernels are in kernels.hpp.  Parity mode's
// kernels and the samplers are chain_api.hip's, the token batches and the fp32 serving chain batch_api.hip's, the Q8 entry points q8_api.hip's, q8_serve_api.hip's and
// q8_spec_api.hip's; ctx.hpp is what the six share.
#include "../../include/rama_hip.h"
#include "kernels.hpp"
#include "ops_kernels.hpp"
#include "ref_kernels.hpp"
#include "attn_wo.hpp"
#include "layer_fused.hpp"
#include "ref_order.hpp"
#include "ctx.hpp"

#ifdef RAMA_CHAIN_HPP
#error "rama_api.hip must not include chain.hpp or topp_pick.hpp: their kernels and g_pred_stats belong to chain_api.hip's code object"
#endif
#ifdef RAMA_PREFILL_MFMA_HPP
#error "rama_api.hip must not include prefill_mfma.hpp: its six non-template kernels would be defined twice, and its GEMMs belong to batch_api.hip's code object"
#endif

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace rama;

extern "C" const float* rama_internal_w13_lookup(const float* w1, const float* w3);   // model.hip
extern "C" const float* rama_internal_tiled_lookup(const float* src);                    // model.hip
extern "C" const float* rama_internal_chain_lookup(const float* a, int rows, int K);     // model.hip
extern "C" int rama_internal_model_ensure(rama_ctx* ctx, const rama_weights* w, int what);       // model.hip: 1 = chain order, 2 = tile order
extern "C" int rama_internal_model_ensure_ptr(rama_ctx* ctx, const float* p, int what);
extern "C" unsigned long long rama_internal_copies_generation();                                           // model.hip: advances whenever a derived weight copy is freed
extern "C" void rama_internal_note_alloc(const float* base, size_t n);                                   // model.hip: the allocation table
extern "C" int rama_internal_forget_range(rama_ctx* ctx, const float* base, size_t n, int freed);      // ... the copies derived from a range go
extern "C" int rama_internal_adopt(rama_ctx* ctx, const rama_config* cfg, const rama_stage* st, const rama_weights* w);
extern "C" const float* rama_internal_chain_view(rama_ctx* ctx, const float* a, int rows, int K, int capturing);

// ---------------------------------------------------------------- error plumbing

static thread_local std::string g_err;

const char* rama_last_error(void) { return g_err.c_str(); }

int fail(int code, const char* what, const char* file, int line) {
    char buf[512];
    if (code > 0)
        snprintf(buf, sizeof buf, "%s: %s (hipError %d) at %s:%d", what, hipGetErrorString((hipError_t)code), code, file, line);
    else
        snprintf(buf, sizeof buf, "%s (rama error %d) at %s:%d", what, code, file, line);
    g_err = buf;
    return code;
}

// ---------------------------------------------------------------- context

void destroy_graph(CapturedGraph& g) {
    if (g.exec) hipGraphExecDestroy(g.exec);
    if (g.graph) hipGraphDestroy(g.graph);
    g = CapturedGraph();
}

int set_device(rama_ctx* c) { HIPCHK(hipSetDevice(c->device)); return 0; }

// internal accessors for the library's other translation units (pipe.hip); not in the C ABI header.  (The recorded 1:1 ops are issued by whatever
// enters the library next -- flush_pending, "the 1:1 op recorder" below: first statement of every entry point that enqueues, synchronises or
// changes a setting.)
extern "C" void* rama_internal_stream(rama_ctx* c) { if (c && RAMA_PENDING(c)) (void)flush_pending(c); return c ? (void*)c->stream : nullptr; }
extern "C" int rama_internal_device(rama_ctx* c) { return c ? c->device : 0; }
// launches made for the 1:1 op entries and by flush_pending since the last reset (PendingOps::op_launches): what tells a test that a fold still
// happens.  Issues nothing that is pending and touches no stream.
extern "C" unsigned long long rama_internal_op_launches(rama_ctx* c, int reset) {
    if (!c) return 0;
    const unsigned long long n = c->rec.op_launches;
    if (reset) c->rec.op_launches = 0;
    return n;
}
// the sampler's device scratch after a rama_sample_topp* call (tests compare the running sums with a
// sequential fp32 cumsum): sorted probabilities, sorted indices, running sums, candidate count
extern "C" void rama_internal_topp_scratch(rama_ctx* c, float** keys, int** vals, float** prefix, int** m) {
    if (c && RAMA_PENDING(c)) (void)flush_pending(c);
    if (keys) *keys = c->topp_keys[1];
    if (vals) *vals = c->topp_vals[1];
    if (prefix) *prefix = c->topp_prefix;
    if (m) *m = c->topp_m;
}

int rama_ctx_create(int device, void* hip_stream, rama_ctx** out) {
    REQUIRE(out, RAMA_EINVAL, "rama_ctx_create: out is NULL");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    REQUIRE(device >= 0 && device < n, RAMA_EINVAL, "rama_ctx_create: no such device");
    HIPCHK(hipSetDevice(device));
    rama_ctx* c = new rama_ctx();
    c->device = device;
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    HIPCHK(hipEventCreate(&c->t0));
    HIPCHK(hipEventCreate(&c->t1));
    HIPCHK(hipMalloc(&c->ctl, sizeof(Ctl)));
    HIPCHK(hipMemset(c->ctl, 0, sizeof(Ctl)));
    c->out_cap = 1 << 16;
    HIPCHK(hipMalloc(&c->out, sizeof(int) * c->out_cap));
    HIPCHK(hipHostMalloc(&c->ring, sizeof(int) * c->out_cap, hipHostMallocMapped));
    memset(c->ring, 0, sizeof(int) * c->out_cap);
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->ring_dev), c->ring, 0));
    c->forced_cap = 1 << 16;
    HIPCHK(hipMalloc(&c->forced, sizeof(int) * c->forced_cap));
    HIPCHK(hipMalloc(&c->argmax_result, sizeof(int)));
    HIPCHK(hipMalloc(&c->attn_counter, sizeof(unsigned)));
    HIPCHK(hipMemset(c->attn_counter, 0, sizeof(unsigned)));
    HIPCHK(hipMalloc(&c->fused_hand, (size_t)kFusedMaxLayers * fused_hand_words(kFusedMaxDim, kFusedMaxHidden) * sizeof(tagged_t)));
    HIPCHK(hipMemset(c->fused_hand, 0, (size_t)kFusedMaxLayers * fused_hand_words(kFusedMaxDim, kFusedMaxHidden) * sizeof(tagged_t)));
    HIPCHK(hipMalloc(&c->fused_epoch, sizeof(unsigned)));
    { const unsigned one = 1; HIPCHK(hipMemcpy(c->fused_epoch, &one, sizeof one, hipMemcpyHostToDevice)); }      // the zeroed vectors carry tag 0
    HIPCHK(hipMalloc(&c->lead_slots, 2 * kLeadSlots * 32 * sizeof(unsigned long long)));      // (the second half: the recorded norms of the 1:1 op path)
    HIPCHK(hipMemset(c->lead_slots, 0, 2 * kLeadSlots * 32 * sizeof(unsigned long long)));
    HIPCHK(hipMalloc(&c->pbar, 4 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(c->pbar, 0, 4 * sizeof(unsigned long long)));
    HIPCHK(hipHostMalloc(&c->pinned_int, sizeof(int) * 4));
    HIPCHK(hipHostMalloc(&c->pinned_tok, sizeof(int) * kMfMaxTok + sizeof(SeqSlot) * kMfMaxTok));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->cu_count = prop.multiProcessorCount;
#define RAMA_FUSED_ATTR(G_, CD_) \
    HIPCHK(hipFuncSetAttribute((const void*)stage_fused_kernel<G_, CD_, 4, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFusedSoloLds)); \
    HIPCHK(hipFuncSetAttribute((const void*)stage_fused_kernel<G_, CD_, 2, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFusedSoloLds));
    RAMA_FUSED_ATTR(16, 2) RAMA_FUSED_ATTR(16, 4) RAMA_FUSED_ATTR(32, 2) RAMA_FUSED_ATTR(32, 4) RAMA_FUSED_ATTR(64, 2) RAMA_FUSED_ATTR(64, 4)
#undef RAMA_FUSED_ATTR
    { const int ri = chain_api_init(c); if (ri) return ri; }      // the same for chain_api.hip's kernels: an attribute reaches the kernels of the translation unit that sets it
    *out = c;
    return 0;
}

void drop_graph(rama_ctx* c) {
    drop_batch_graphs(c);
    for (auto& g : c->gc) { destroy_graph(g.cg); g = GraphCache(); }
    for (auto& e : c->sg) destroy_graph(e.g.cg);
    c->sg.clear();
    drop_q8_graphs(c, nullptr);
}

extern "C" void rama_internal_drop_graphs(rama_ctx* c) { if (c) drop_graph(c); }      // model.hip: before a derived weight copy is freed

int rama_ctx_destroy(rama_ctx* c) {
    if (c && RAMA_PENDING(c)) (void)flush_pending(c);
    if (!c) return 0;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    drop_graph(c);
    for (auto e : c->kp.ev) hipEventDestroy(e);
    hipFree(c->ctl); hipFree(c->out); hipFree(c->forced); hipFree(c->argmax_result); hipFree(c->pbar); hipFree(c->attn_counter); hipFree(c->attn_part); hipFree(c->attn_scores); hipFree(c->fused_hand); hipFree(c->fused_epoch); hipFree(c->lead_slots);
    for (int i = 0; i < 2; i++) { hipFree(c->topp_keys[i]); hipFree(c->topp_vals[i]); }
    hipFree(c->topp_prefix); hipFree(c->topp_m); hipFree(c->topp_err); if (c->ring) hipHostFree(c->ring);
    hipFree(c->topp_bp); hipFree(c->topp_bi); hipFree(c->topp_bcount); hipFree(c->topp_racc);
    hipFree(c->topp_rk); hipFree(c->topp_bm); hipFree(c->topp_approx); hipFree(c->topp_dist); hipFree(c->topp_stats);
    release_batch(c);
    release_q8(c);
    hipFree(c->tb.keys); hipFree(c->tb.vals); hipFree(c->tb.bp); hipFree(c->tb.bi); hipFree(c->tb.rk); hipFree(c->tb.bm);
    hipFree(c->tb.bcount); hipFree(c->tb.stats); hipFree(c->tb.m); hipFree(c->tb.rows_dev);
    hipHostFree(c->pinned_int); hipHostFree(c->pinned_tok);
    hipEventDestroy(c->t0); hipEventDestroy(c->t1);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

// The launches that hand data over INSIDE a kernel (attention+Wo, the one-launch stage) bound every wait and report a wait that gave up
// through the error word at pbar[1]; their results are then invalid.  Every synchronising exit reads the word -- once the stream is idle
// -- fails the call and clears it, so that neither garbage logits leave with rc 0 nor a stale word makes every later launch give up.
int handoff_check(rama_ctx* c) {
    { const int rt = topp_dist_check(c); if (rt) return rt; }
    if (!c->handoff_dirty || !c->pbar) return 0;
    unsigned long long perr = 0;
    HIPCHK(hipMemcpyAsync(&perr, c->pbar + 1, sizeof perr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->handoff_dirty = false;
    if (perr != 0) {
        hipMemsetAsync(c->pbar, 0, 4 * sizeof(unsigned long long), c->stream);   // counter, error word, base: start over
        hipStreamSynchronize(c->stream);
        return fail(RAMA_EINVAL, perr >= 0x3000ull ? "one-launch stage: a hand-off timed out" : "attention+Wo launch: hand-off timed out", __FILE__, __LINE__);
    }
    return 0;
}

int replay_graph(rama_ctx* c, const CapturedGraph& g) {
    HIPCHK(hipGraphLaunch(g.exec, c->stream));
    if (g.handoff) c->handoff_dirty = true;
    return 0;
}

int rama_sync(rama_ctx* c) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "rama_sync: ctx is NULL");
    HIPCHK(hipStreamSynchronize(c->stream));
    return handoff_check(c);
}

// 0: everything enqueued on the context's stream has run; 1: work is still running; anything else: the stream has failed (the error
// is also recorded for rama_last_error).  Never blocks -- what a host loop that polls the token rings uses to know when to stop.
int rama_stream_query(rama_ctx* c) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "rama_stream_query: ctx is NULL");
    const hipError_t e = hipStreamQuery(c->stream);
    if (e == hipSuccess) return 0;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return 1; }
    return fail((int)e, "hipStreamQuery", __FILE__, __LINE__);
}

int rama_device_info(rama_ctx* c, char name[64], int* cus, size_t* hbm) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, c->device));
    if (name) {   // marketing name needs amdgpu.ids, absent on some boxes: fall back to the ISA name
        strncpy(name, prop.name[0] ? prop.name : prop.gcnArchName, 63);
        name[63] = 0;
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm) *hbm = prop.totalGlobalMem;
    return 0;
}

// ---------------------------------------------------------------- memory

int rama_alloc_f32(rama_ctx* c, size_t n, float** out) {
    RAMA_ENTER(c);
    REQUIRE(c && out, RAMA_EINVAL, "rama_alloc_f32: NULL argument");
    if (set_device(c)) return 1;
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(float)));
    HIPCHK(hipMemsetAsync(p, 0, std::max<size_t>(n, 1) * sizeof(float), c->stream));
    *out = (float*)p;
    rama_internal_note_alloc((const float*)p, std::max<size_t>(n, 1));
    return 0;
}

int rama_copy_h2d_f32(rama_ctx* c, float* dst, const float* host, size_t n) {
    RAMA_ENTER(c);
    REQUIRE(c && (n == 0 || (dst && host)), RAMA_EINVAL, "rama_copy_h2d_f32: NULL argument");
    if (n == 0) return 0;
    { const int rf = rama_internal_forget_range(c, dst, n, 0); if (rf) return rf; }      // copies derived from what is overwritten here
    HIPCHK(hipMemcpyAsync(dst, host, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // htod_sync_copy semantics (hbm.rs:14-16)
    return 0;
}

int rama_upload_f32(rama_ctx* c, const float* host, size_t n, float** out) {
    RAMA_ENTER(c);
    int rc = rama_alloc_f32(c, n, out);
    if (rc) return rc;
    return rama_copy_h2d_f32(c, *out, host, n);
}

int rama_download_f32(rama_ctx* c, const float* src, size_t n, float* host) {
    RAMA_ENTER(c);
    REQUIRE(c && (n == 0 || (src && host)), RAMA_EINVAL, "rama_download_f32: NULL argument");
    if (n == 0) return 0;
    HIPCHK(hipMemcpyAsync(host, src, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return handoff_check(c);
}

int rama_free(rama_ctx* c, void* p) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    if (!p) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    { const int rf = rama_internal_forget_range(c, (const float*)p, 1, 1); if (rf) return rf; }      // (any range inside the allocation: entries are matched by overlap with it below)
    HIPCHK(hipFree(p));
    return 0;
}

// ---------------------------------------------------------------- launch helpers

// Matvec workgroup geometry: R_ rows (R2_ (w1,w3) row pairs) per workgroup of NW_ waves, CH_
// 1-KiB chunks per wave per step.  Geometry 3 (4 rows x 8 waves x 2 chunks) ships: in the
// full llama2-7B decode it gives 233 tok/s vs 223 / 221 / 231 for 0 / 1 / 2 (tools/tune.py).
// The bare-matvec sweep (tools/gemv_bench.hip) prefers 2 rows per workgroup, but the kernels
// with rmsnorm folded in re-read x and the norm gain per workgroup, which 4 rows amortise.
// The others stay selectable for A/B runs through rama_set_tuning(ctx, "geom", g).
#define DISPATCH_GEOM(c, KERNEL_CALL)                                                                          \
    switch ((c)->tune_geom) {                                                                                  \
        case 1: { constexpr int R_ = 2, R2_ = 1, CH_ = 4, NW_ = 4; (void)R_; (void)R2_; KERNEL_CALL; } break;  \
        case 2: { constexpr int R_ = 4, R2_ = 2, CH_ = 4, NW_ = 4; (void)R_; (void)R2_; KERNEL_CALL; } break;  \
        case 0: { constexpr int R_ = 2, R2_ = 1, CH_ = 2, NW_ = 8; (void)R_; (void)R2_; KERNEL_CALL; } break;  \
        case 4: { constexpr int R_ = 8, R2_ = 4, CH_ = 2, NW_ = 8; (void)R_; (void)R2_; KERNEL_CALL; } break;  \
        default: { constexpr int R_ = 4, R2_ = 2, CH_ = 2, NW_ = 8; (void)R_; (void)R2_; KERNEL_CALL; } break; \
    }

static int check_matvec_shape(size_t width, size_t rows) {
    REQUIRE(width % 4 == 0, RAMA_EINVAL, "matmul: width % 4 != 0 (the reference CPU body panics here, cpu.rs:142-143)");
    REQUIRE(width > 0 && rows > 0, RAMA_EINVAL, "matmul: empty shape");
    REQUIRE((double)width * (double)rows * 4.0 < 2147483648.0, RAMA_EINVAL, "matmul: matrix >= 2 GiB, split it by layer");
    return 0;
}

static bool use_solo(const rama_ctx* c, int K) { return c->tune_solo < 0 ? K <= 2048 : c->tune_solo != 0; }

// plain W.x (EPI_STORE) or x += W.y (EPI_RESID)
template <bool NORM, int EPI>
static int launch_rows(rama_ctx* c, float* o, const float* W, const float* x, const float* nw, int K, int rows) {
    int rc = check_matvec_shape(K, rows);
    if (rc) return rc;
    GemvParams p{};
    p.w[0] = W; p.x = x; p.nw = nw; p.o[0] = o; p.K = K; p.rows = rows; p.nmat = 1;
    if (use_solo(c, K)) {      // small-K: one wave per 4 rows (kernels.hpp gemv_rows_solo)
        const dim3 grid(((rows + 3) / 4 + kSoloWaves - 1) / kSoloWaves), block(kSoloWaves * 64);
        if (K <= 512) RAMA_LAUNCH(c, (gemv_rows_solo<4, 2, NORM, EPI>), grid, block, 0, p);
        else RAMA_LAUNCH(c, (gemv_rows_solo<4, 4, NORM, EPI>), grid, block, 0, p);
        LAUNCHCHK();
        return 0;
    }
    if (!NORM && EPI == EPI_RESID && c->tune_geom == 3 && c->tune_resid_r2) {
        // the residual matvecs (Wo, W2) read no rmsnorm gain, so a 2-row workgroup's re-read of
        // x is cheap and the finer grain balances better; rows wider than
        // 8192 floats (W2) can also spread over 16 waves (resid_r2 = 2 / 3)
        if (K > 8192 && c->tune_resid_r2 == 2) RAMA_LAUNCH(c, (gemv_rows<2, 1, 16, NORM, EPI>), dim3((rows + 1) / 2), dim3(16 * 64), 0, p);
        else if (K > 8192 && c->tune_resid_r2 == 3) RAMA_LAUNCH(c, (gemv_rows<2, 4, 16, NORM, EPI>), dim3((rows + 1) / 2), dim3(16 * 64), 0, p);
        else RAMA_LAUNCH(c, (gemv_rows<2, 2, 8, NORM, EPI>), dim3((rows + 1) / 2), dim3(8 * 64), 0, p);
        LAUNCHCHK();
        return 0;
    }
    DISPATCH_GEOM(c, RAMA_LAUNCH(c, (gemv_rows<R_, CH_, NW_, NORM, EPI>), dim3((rows + R_ - 1) / R_), dim3(NW_ * 64), 0, p));
    LAUNCHCHK();
    return 0;
}
// infer.rs:49-51 for one token, for batch_api.hip (rama_prefill's last position): the gemv_rows instantiations stay this translation unit's
int launch_classifier(rama_ctx* c, float* logits, const float* wcls, const float* x, const float* gain, int dim, int vocab) {
    return launch_rows<true, EPI_STORE>(c, logits, wcls, x, gain, dim, vocab);
}

// ---------------------------------------------------------------- reference-order launches (ref_order.hpp)

static int launch_matvec_ref(rama_ctx* c, int nmat, float* const o[3], const float* const W[3], const float* x, int K, int rows) {
    REQUIRE(K % 4 == 0 && K > 0 && rows > 0, RAMA_EINVAL, "matmul: width % 4 != 0 (the reference CPU body panics here, cpu.rs:142-143)");
    RefMatParams p{};
    for (int m = 0; m < nmat; m++) { p.w[m] = W[m]; p.o[m] = o[m]; }
    p.x = x; p.K = K; p.rows = rows; p.lane_reduce = c->tune_lane_reduce;
    hipLaunchKernelGGL(matvec_ref_kernel, dim3((rows + 63) / 64, nmat), dim3(64), 0, c->stream, p);
    LAUNCHCHK();
    return 0;
}
static int launch_matvec_ref1(rama_ctx* c, float* o, const float* W, const float* x, int K, int rows) {
    float* const oo[3] = {o, nullptr, nullptr};
    const float* const ww[3] = {W, nullptr, nullptr};
    return launch_matvec_ref(c, 1, oo, ww, x, K, rows);
}
int launch_rmsnorm_ref(rama_ctx* c, float* o, const float* x, const float* w, int n) {
    REQUIRE((size_t)n * sizeof(float) <= 64 * 1024, RAMA_EUNSUP, "rmsnorm (reference order): vector longer than 16384");
    hipLaunchKernelGGL(rmsnorm_ref_kernel, dim3(1), dim3(1024), (size_t)n * sizeof(float), c->stream, o, x, w, n);
    LAUNCHCHK();
    return 0;
}
int launch_attention_ref(rama_ctx* c, float* xb, float* att, const float* q, const float* kc_layer, const float* vc_layer,
                                const Ctl* ctl, int pos, int dim, int head_size, int seq_len, int n_heads) {
    REQUIRE((size_t)seq_len * sizeof(float) <= 64 * 1024, RAMA_EUNSUP, "attention (reference order): seq_len longer than 16384");
    RefAttnParams p{};
    p.q = q; p.kc = kc_layer; p.vc = vc_layer; p.att = att; p.xb = xb; p.ctl = ctl; p.pos_val = pos;
    p.dim = dim; p.head_size = head_size; p.seq_len = seq_len;
    hipLaunchKernelGGL(attention_ref_kernel, dim3(n_heads), dim3(1024), (size_t)seq_len * sizeof(float), c->stream, p);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------- the 1:1 op recorder (rama_ctx::rec; what may be pending together: ctx.hpp PendingOps)

// every launch for a 1:1 op entry or for flush_pending is counted (rama_internal_op_launches): a kernel of this translation unit ...
#define OP_LAUNCH(c, kernel, grid, block, shm, ...) do { hipLaunchKernelGGL(kernel, grid, block, shm, (c)->stream, __VA_ARGS__); (c)->rec.op_launches++; LAUNCHCHK(); } while (0)
// ... or a launcher's one launch, by its return code
static int counted(rama_ctx* c, int rc) { if (!rc) c->rec.op_launches++; return rc; }

static bool may_record(const rama_ctx* c, int tune_switch) { return tune_switch && c->own_stream; }
// rama_rmsnorm records only on CAPTURE_NONE; rama_matmul takes a failed query (CAPTURE_UNKNOWN) for a capture
enum Capture { CAPTURE_NONE, CAPTURE_ON, CAPTURE_UNKNOWN };
static Capture stream_capture(rama_ctx* c) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess) return CAPTURE_UNKNOWN;
    return cs == hipStreamCaptureStatusNone ? CAPTURE_NONE : CAPTURE_ON;
}
struct Range { const float* p; size_t n; };
static bool apart_from(const float* p, size_t n, std::initializer_list<Range> others) {
    for (const Range& r : others) if (ranges_overlap(p, n, r.p, r.n)) return false;
    return true;
}

// the launches an entry and the flush of its record share: the reference's rounding order in parity mode, else the fast kernel
static int launch_sinu(rama_ctx* c, float* t, size_t n) {
    if (c->tune_ref_order) OP_LAUNCH(c, sinu_ref_kernel, dim3(ew_grid(n)), dim3(256), 0, t, n);
    else OP_LAUNCH(c, sinu_kernel, dim3(ew_grid(n)), dim3(256), 0, t, n);
    return 0;
}
static int launch_copy(rama_ctx* c, float* t, const float* s, size_t n) {
    OP_LAUNCH(c, copy_kernel, dim3(ew_grid(n)), dim3(256), 0, t, s, n);
    return 0;
}
// `count` consecutive heads are one vector of count x head_size floats
static int launch_rope_run(rama_ctx* c, float* q, float* k, const float* pr, const float* pi, int hs, int count) {
    const int dim = count * hs, n = dim / 2;
    if (c->tune_ref_order) OP_LAUNCH(c, rope_ref_kernel, dim3((n + 63) / 64), dim3(64), 0, q, k, (const float*)nullptr, pr, pi, dim, hs, (float*)nullptr, (float*)nullptr);
    else OP_LAUNCH(c, apply_position_heads_kernel, dim3((n + 63) / 64), dim3(64), 0, q, k, pr, pi, hs, dim);
    return 0;
}

// the pending run of matmuls as the parameters of its chain-order launch
static ChainParams run_params(const PendingOps& r) {
    ChainParams p{};
    for (int i = 0; i < r.mm.count; i++) { p.w[i] = r.mm.w[i]; p.o[i] = r.mm.o[i]; }
    p.x = r.mm.x; p.K = r.mm.K; p.rows = r.mm.rows; p.nmat = r.mm.count;
    return p;
}
// THE launch of a chain run.  with_norm: the run reads the recorded norm's output, so the norm rides in the run's launch as its leader workgroup,
// which also stores that output; the leader's word is the next of the op path's range, and when the range wraps every word of it carries this
// epoch: the next one.  (The one place that advances PendingOps::lead_next.)
static int launch_run(rama_ctx* c, ChainParams& p, int epi, bool with_norm) {
    PendingOps& r = c->rec;
    if (!with_norm) return counted(c, launch_chain(c, p, epi));
    r.nrm.on = false;
    p.x = r.nrm.x; p.nw = r.nrm.w; p.xout = r.nrm.o;
    p.lead = c->lead_slots + 32 * (kLeadSlots + r.lead_next); p.epoch = c->fused_epoch; p.err = c->pbar + 1;
    const int rc = counted(c, launch_chain(c, p, epi, CNORM_LEAD));
    if (rc) return rc;
    if (++r.lead_next == kLeadSlots) {
        r.lead_next = 0;
        OP_LAUNCH(c, fused_epoch_kernel, dim3(1), dim3(1), 0, c->fused_epoch);
    }
    return 0;
}

// what is pending, record by record.  flush_norm: no run of matmuls took the norm; flush_mm: the run as one chain-order launch, and the recorded norm in
// that launch or in front of it; flush_rope: the rotations as one launch; flush_ew: the elementwise op by itself
static int flush_norm(rama_ctx* c) {
    auto& n = c->rec.nrm;
    return std::exchange(n.on, false) ? counted(c, launch_rmsnorm_chain(c, n.o, n.x, n.w, n.n, nullptr)) : 0;
}
static int flush_mm(rama_ctx* c) {
    PendingOps& r = c->rec;
    if (!(r.mm.count && r.mm.norm)) { const int rn = flush_norm(c); if (rn) return rn; }
    if (!r.mm.count) return 0;
    ChainParams p = run_params(r);
    r.mm.count = 0;
    return launch_run(c, p, CEPI_STORE, std::exchange(r.mm.norm, false));
}
static int flush_rope(rama_ctx* c) {
    auto& r = c->rec.rope;
    const int count = std::exchange(r.count, 0);
    return count ? launch_rope_run(c, r.q, r.k, r.pr, r.pi, r.hs, count) : 0;
}
static int flush_ew(rama_ctx* c) {
    auto& e = c->rec.ew;
    const int kind = std::exchange(e.kind, 0);
    return !kind ? 0 : kind == 1 ? launch_sinu(c, e.t, e.n) : launch_copy(c, e.t, e.s, e.n);
}
// everything pending, in the order it can have been recorded: a norm and the run of matmuls on it, the rotations of that run's q and k, a copy
int flush_pending(rama_ctx* c) { int rf = flush_mm(c); if (!rf) rf = flush_rope(c); if (!rf) rf = flush_ew(c); return rf; }

// ---- the folds: when a call joins what is recorded (r) instead of issuing it

// [r5] array_add(t, s) where s is the output of the one recorded matmul (infer.rs:35-37, :46-47): ONE launch with the residual epilogue (product stored, t += product)
static bool add_is_residual_of_run(const rama_ctx* c, const PendingOps& r, const float* t, const float* s, size_t n) {
    return r.mm.count == 1 && !r.mm.norm && !r.nrm.on && !r.rope.count && !r.ew.kind && c->tune_ref_order && c->tune_resid_fold && s == r.mm.o[0] && n == (size_t)r.mm.rows &&
           aligned16(t) && apart_from(t, n, {{r.mm.x, (size_t)r.mm.K}, {s, n}});
}
// array_mult(t, s) on the vector of the recorded sinu: one launch for both
static bool mult_takes_sinu(const PendingOps& r, const float* t, const float* s, size_t n) {
    return r.ew.kind == 1 && !r.rope.count && !r.mm.count && r.ew.t == t && r.ew.n == n && n && !ranges_overlap(s, n, t, n);
}
// copy_from_slice(t, s) behind a recorded copy that it neither reads nor overwrites: one launch for both
static bool copy_pairs_with_copy(const PendingOps& r, const float* t, const float* s, size_t n) {
    return r.ew.kind == 2 && !r.rope.count && !r.mm.count && n && apart_from(r.ew.t, r.ew.n, {{s, n}, {t, n}}) && apart_from(t, n, {{r.ew.s, r.ew.n}, {s, n}});
}
// [r5] infer.rs:20-33 as the fused entry runs it: a pending run of three matmuls (a recorded norm in front, perhaps), every head of its first two outputs
// rotated, and then its second and third outputs copied into cache rows -- ONE launch with the Wq|Wk|Wv epilogue.  The first copy is recorded
// (copy_opens_qkv_fold), the second issues the launch (copy_closes_qkv_fold); a copy of that shape that is neither issues what is pending in program order.
static bool copy_meets_rotated_qkv_run(const rama_ctx* c, const PendingOps& r, size_t n) {
    return r.mm.count == 3 && r.rope.count && c->tune_qkv_fold && c->tune_ref_order && n == (size_t)r.mm.rows && r.rope.count * r.rope.hs == r.mm.rows;
}
static bool apart_from_qkv_run(const PendingOps& r, const float* p, size_t n) {      // from everything that launch reads or writes besides
    const size_t rows = (size_t)r.mm.rows, hh = (size_t)r.rope.hs / 2;
    return apart_from(p, n, {{r.mm.o[0], rows}, {r.mm.o[1], rows}, {r.mm.o[2], rows}, {r.mm.x, (size_t)r.mm.K}, {r.rope.pr, hh}, {r.rope.pi, hh}}) &&
           (!r.mm.norm || apart_from(p, n, {{r.nrm.x, (size_t)r.nrm.n}, {r.nrm.w, (size_t)r.nrm.n}}));
}
static bool copy_opens_qkv_fold(const rama_ctx* c, const PendingOps& r, const float* t, const float* s, size_t n) {
    return !r.ew.kind && s == r.mm.o[1] && aligned16(t) && apart_from_qkv_run(r, t, n) && may_record(c, c->tune_ew_batch);
}
static bool copy_closes_qkv_fold(const PendingOps& r, const float* t, const float* s, size_t n) {
    const size_t hh = (size_t)r.rope.hs / 2;
    return r.ew.kind == 2 && r.ew.s == r.mm.o[1] && r.ew.n == n && s == r.mm.o[2] && aligned16(t) && apart_from_qkv_run(r, t, n) && !ranges_overlap(t, n, r.ew.t, n) &&
           apart_from(r.rope.pr, hh, {{r.mm.o[0], n}, {r.mm.o[1], n}, {r.mm.o[2], n}}) && apart_from(r.rope.pi, hh, {{r.mm.o[0], n}, {r.mm.o[1], n}, {r.mm.o[2], n}});
}
static int launch_qkv_fold(rama_ctx* c, float* value_row) {
    PendingOps& r = c->rec;
    ChainParams p = run_params(r);
    p.fr = r.rope.pr; p.fi = r.rope.pi; p.head_size = r.rope.hs; p.kc = r.ew.t; p.vc = value_row; p.pos_val = 0;      // (the table rows and cache rows of this position themselves)
    r.mm.count = 0; r.rope.count = 0; r.ew.kind = 0;
    return launch_run(c, p, CEPI_QKV, std::exchange(r.mm.norm, false));
}
// apply_position(q, k) that starts to rotate the first two outputs of a pending run of three matmuls, or goes on rotating them: the run stays pending
static bool rope_is_on_qkv_run(const rama_ctx* c, const PendingOps& r, const float* q, const float* k, size_t head_size) {
    return r.mm.count == 3 && c->tune_qkv_fold && !r.ew.kind && may_record(c, c->tune_rope_batch) && head_size % 2 == 0 && r.mm.rows % (int)head_size == 0 &&
           (r.rope.count ? true : (q == r.mm.o[0] && k == r.mm.o[1]));
}
// apply_position on the head behind the recorded run's last, with the same table rows (and inside the outputs of a pending run of matmuls)
static bool rope_extends_run(const PendingOps& r, const float* q, const float* k, const float* pr, const float* pi, int hs) {
    return r.rope.count && r.rope.count < 4096 && hs == r.rope.hs && pr == r.rope.pr && pi == r.rope.pi && q == r.rope.q + (size_t)r.rope.count * hs &&
           k == r.rope.k + (size_t)r.rope.count * hs && (!r.mm.count || (r.rope.count + 1) * hs <= r.mm.rows);
}
// a parity-mode rmsnorm the leader workgroup of a chain launch can carry: not in place, 64 <= n <= 4096 in whole 16-float blocks, default geometry, no
// kernel class being timed (rama_rmsnorm asks last whether the stream is capturing)
static bool norm_may_ride(const rama_ctx* c, const float* o, const float* x, const float* w, size_t n) {
    return c->tune_ref_order && c->tune_chain && rmsnorm_chain_ok(n) && c->tune_norm_fold && c->tune_chain_lead && may_record(c, c->tune_matmul_batch) && c->tune_chain_d <= 0 &&
           c->tune_chain_lead_w <= 0 && c->kp.kernel_id < 0 && n % 16 == 0 && n <= 4096 && n >= 64 && aligned16(x) && aligned16(w) && aligned16(o) && (o + n <= x || x + n <= o) && c->lead_slots && c->pbar;
}
// matmul(o, a, b) with the activations and the shape of the pending run of one or two: the run's next member, if its output allows (below)
static bool matmul_joins_run(const rama_ctx* c, const PendingOps& r, const float* b, size_t width, size_t o_rows, size_t o_cols) {
    return r.mm.count && r.mm.count < 3 && c->tune_ref_order && o_cols == 1 && r.mm.x == b && r.mm.K == (int)width && r.mm.rows == (int)o_rows;
}
// the recorded norm rides with a run on its output: the run this matmul joins has taken it, or this matmul opens the run
static bool run_takes_norm(const PendingOps& r, const float* b, size_t width) { return r.nrm.on && (r.mm.count ? r.mm.norm : (b == r.nrm.o && (int)width == r.nrm.n)); }
// an output that overlaps the activations, an output of the run, or the input of the norm the run takes (which the launch then reads) is no member
static bool output_clashes_with_run(const PendingOps& r, const float* o, const float* b, size_t width, size_t o_rows, bool takes_norm) {
    bool clash = ranges_overlap(o, o_rows, b, width);
    for (int i = 0; i < r.mm.count && !clash; i++) clash = ranges_overlap(o, o_rows, r.mm.o[i], o_rows);
    return clash || (takes_norm && ranges_overlap(o, o_rows, r.nrm.x, (size_t)r.nrm.n));
}

// ---------------------------------------------------------------- Device<T> ops, 1:1
// Each entry: argument checks, RAMA_WRITES, the folds that apply to the op, else what is pending is issued, else the call is recorded or launched.
// Where an entry's order of REQUIRE, RAMA_WRITES and the flush differs from that, it decides which error a bad call returns and whether pending work
// is issued in front of the error: kept as it was.

int rama_array_add(rama_ctx* c, float* t, const float* s, size_t n) {
    REQUIRE(c && (n == 0 || (t && s)), RAMA_EINVAL, "array_add: NULL argument");      // (in front of RAMA_ENTER, unlike rama_sinu: a bad call leaves what is pending pending.  Looks accidental; kept)
    RAMA_WRITES(c, t, n);
    if (add_is_residual_of_run(c, c->rec, t, s, n)) {
        ChainParams p = run_params(c->rec);
        p.resid = t;
        c->rec.mm.count = 0;
        return launch_run(c, p, CEPI_RESID, false);
    }
    RAMA_ENTER(c);
    if (!n) return 0;
    OP_LAUNCH(c, array_add_kernel, dim3(ew_grid(n)), dim3(256), 0, t, s, n);
    return 0;
}
int rama_array_mult(rama_ctx* c, float* t, const float* s, size_t n) {
    REQUIRE(c && (n == 0 || (t && s)), RAMA_EINVAL, "array_mult: NULL argument");      // (as rama_array_add)
    RAMA_WRITES(c, t, n);
    if (mult_takes_sinu(c->rec, t, s, n)) {
        c->rec.ew.kind = 0;
        if (c->tune_ref_order) OP_LAUNCH(c, sinu_mult_ref_kernel, dim3(ew_grid(n)), dim3(256), 0, t, s, n);
        else OP_LAUNCH(c, sinu_mult_kernel, dim3(ew_grid(n)), dim3(256), 0, t, s, n);
        return 0;
    }
    RAMA_ENTER(c);
    if (!n) return 0;
    OP_LAUNCH(c, array_mult_kernel, dim3(ew_grid(n)), dim3(256), 0, t, s, n);
    return 0;
}
int rama_sinu(rama_ctx* c, float* o, size_t n) {
    RAMA_ENTER(c);      // (no fold applies: what is pending goes first, in front of the argument check)
    REQUIRE(c && (n == 0 || o), RAMA_EINVAL, "sinu: NULL argument");
    RAMA_WRITES(c, o, n);
    if (!n) return 0;
    if (may_record(c, c->tune_ew_batch)) { c->rec.ew = {1, o, nullptr, n}; return 0; }      // recorded: the product that usually follows takes it along
    return launch_sinu(c, o, n);
}
int rama_copy_from_slice(rama_ctx* c, float* t, const float* s, size_t n) {
    REQUIRE(c && (n == 0 || (t && s)), RAMA_EINVAL, "copy_from_slice: NULL argument");      // (as rama_array_add)
    RAMA_WRITES(c, t, n);
    if (copy_meets_rotated_qkv_run(c, c->rec, n)) {
        if (copy_opens_qkv_fold(c, c->rec, t, s, n)) { c->rec.ew = {2, t, s, n}; return 0; }
        if (copy_closes_qkv_fold(c->rec, t, s, n)) return launch_qkv_fold(c, t);
        { const int rf = flush_pending(c); if (rf) return rf; }
    }
    if (copy_pairs_with_copy(c->rec, t, s, n)) {
        PendingOps& r = c->rec;
        r.ew.kind = 0;
        OP_LAUNCH(c, copy2_kernel, dim3(ew_grid(n + r.ew.n)), dim3(256), 0, r.ew.t, r.ew.s, r.ew.n, t, s, n);
        return 0;
    }
    RAMA_ENTER(c);
    if (!n) return 0;
    if (may_record(c, c->tune_ew_batch) && !ranges_overlap(t, n, s, n)) { c->rec.ew = {2, t, s, n}; return 0; }      // recorded: one more copy may follow
    return launch_copy(c, t, s, n);
}
int rama_rmsnorm(rama_ctx* c, float* o, const float* x, const float* w, size_t n) {
    RAMA_ENTER(c);      // (as rama_sinu)
    REQUIRE(c && o && x && w && n > 0, RAMA_EINVAL, "rmsnorm: bad argument");
    RAMA_WRITES(c, o, n);
    if (norm_may_ride(c, o, x, w, n)) {
        if (stream_capture(c) == CAPTURE_NONE) { c->rec.nrm = {o, x, w, (int)n, true}; return 0; }      // recorded: the run of matmuls on `o` carries it (launch_run)
        (void)hipGetLastError();
    }
    if (c->tune_ref_order) return counted(c, c->tune_chain && rmsnorm_chain_ok(n) ? launch_rmsnorm_chain(c, o, x, w, (int)n, nullptr) : launch_rmsnorm_ref(c, o, x, w, (int)n));
    OP_LAUNCH(c, rmsnorm_kernel, dim3(1), dim3(1024), 0, o, x, w, (int)n);
    return 0;
}
int rama_apply_position(rama_ctx* c, float* q, float* k, const float* pr, const float* pi, size_t head_size) {
    REQUIRE(c && q && k && pr && pi && head_size >= 2, RAMA_EINVAL, "apply_position: bad argument");      // (as rama_array_add)
    RAMA_WRITES(c, q, head_size); RAMA_WRITES(c, k, head_size);
    PendingOps& r = c->rec;
    // whatever was recorded before this call comes first -- except a run of rotations, which may go on, and a run of three matmuls that this call rotates
    if (!rope_is_on_qkv_run(c, r, q, k, head_size) && (r.mm.count | r.ew.kind | (int)r.nrm.on)) { const int rm = flush_pending(c); if (rm) return rm; }
    if (may_record(c, c->tune_rope_batch) && head_size % 2 == 0 && head_size <= 4096) {
        const int hs = (int)head_size;
        if (rope_extends_run(r, q, k, pr, pi, hs)) { r.rope.count++; return 0; }
        // (a new run: EVERYTHING pending is issued, a run of three matmuls that this call starts to rotate too -- so the rotations of a run are
        // recorded only once the run has gone, and rama_copy_from_slice never meets a run with its rotations.  Kept as it was: DESIGN.md 3.6)
        const int rf = flush_pending(c); if (rf) return rf;
        r.rope = {q, k, pr, pi, hs, 1};
        return 0;
    }
    { const int rf = flush_pending(c); if (rf) return rf; }
    if (c->tune_ref_order) return launch_rope_run(c, q, k, pr, pi, (int)head_size, 1);      // (one head as a run of one: the same launch)
    const int n = (int)(head_size / 2);
    OP_LAUNCH(c, apply_position_kernel, dim3((n + 63) / 64), dim3(64), 0, q, k, pr, pi, (int)head_size);
    return 0;
}
int rama_matmul(rama_ctx* c, float* o, const float* a, const float* b, size_t width, size_t o_rows, size_t o_cols) {
    if (c && (c->rec.rope.count | c->rec.ew.kind)) { const int rf = flush_pending(c); if (rf) return rf; }      // (in front of the argument checks; a pending run of matmuls may be extended by this call, a recorded norm taken along: below)
    REQUIRE(c && o && a && b, RAMA_EINVAL, "matmul: NULL argument");
    REQUIRE(o_cols >= 1, RAMA_EINVAL, "matmul: o_cols == 0");
    RAMA_WRITES(c, o, o_rows * o_cols);
    int rc = check_matvec_shape(width, o_rows);
    if (rc) { (void)flush_mm(c); return rc; }
    PendingOps& r = c->rec;
    if (!matmul_joins_run(c, r, b, width, o_rows, o_cols) && r.mm.count) { rc = flush_mm(c); if (rc) return rc; }      // (no run pending: a recorded norm stays, this call may open the run that takes it)
    if (c->tune_ref_order && o_cols == 1) {
        // a layer-aligned view of a resident model's matrix streams the model's chain-order copy
        if (c->tune_chain && width % 16 == 0 && width <= 16000 && aligned16(b)) {
            rc = rama_internal_model_ensure_ptr(c, a, 1); if (rc) return rc;
            // ... and a matrix that belongs to no model -- uploaded by itself (hbm.rs:14-16), or a view no model copy covers (w1, w3: a model keeps
            // them interleaved) -- gets a chain-order copy of its own on first use ("chain_views"; freed with the tensor: rama_free)
            const bool capturing = stream_capture(c) != CAPTURE_NONE;
            if (const float* ch = c->tune_chain_views ? rama_internal_chain_view(c, a, (int)o_rows, (int)width, capturing ? 1 : 0) : rama_internal_chain_lookup(a, (int)o_rows, (int)width)) {
                // [r5] recorded, not launched: the next call extends the run (same activations, same shape, an output that overlaps nothing of the run) or
                // issues it.  A run is one launch over all its row groups.
                const bool takes_norm = run_takes_norm(r, b, width);
                if (may_record(c, c->tune_matmul_batch) && !capturing && !output_clashes_with_run(r, o, b, width, o_rows, takes_norm)) {
                    if (!r.mm.count) {
                        r.mm.x = b; r.mm.K = (int)width; r.mm.rows = (int)o_rows; r.mm.norm = takes_norm;
                        if (!takes_norm) { rc = flush_norm(c); if (rc) return rc; }
                    }
                    r.mm.w[r.mm.count] = ch; r.mm.o[r.mm.count] = o; r.mm.count++;
                    if (r.mm.count == 3 && !(c->tune_qkv_fold && c->tune_rope_batch && c->tune_ew_batch)) return flush_mm(c);      // (else: the rotations and cache copies may follow)
                    return 0;
                }
                rc = flush_mm(c); if (rc) return rc;
                ChainParams p{};
                p.w[0] = ch; p.o[0] = o; p.x = b; p.K = (int)width; p.rows = (int)o_rows; p.nmat = 1;
                return launch_run(c, p, CEPI_STORE, false);
            }
        }
        rc = flush_mm(c); if (rc) return rc;
        return counted(c, launch_matvec_ref1(c, o, a, b, (int)width, (int)o_rows));
    }
    // (none of the paths below records: whatever is pending -- a parity-mode Device::rmsnorm whose output this call may read -- is issued first)
    rc = flush_mm(c); if (rc) return rc;
    if (o_cols != 1) {   // forward() never takes this path (o_cols is always 1, infer.rs:20-51)
        size_t n = o_rows * o_cols;
        if (c->tune_ref_order) {      // the reference's rounding order for this shape too (cpu.rs:137-151)
            REQUIRE(width % 4 == 0, RAMA_EINVAL, "matmul: width % 4 != 0 (the reference CPU body panics here, cpu.rs:142-143)");
            OP_LAUNCH(c, matmul_cols_ref_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, o, a, b, (int)width, (int)o_rows, (int)o_cols, c->tune_lane_reduce);
            return 0;
        }
        OP_LAUNCH(c, matmul_generic, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, o, a, b, (int)width, (int)o_rows, (int)o_cols);
        return 0;
    }
    if (!aligned16(a) || !aligned16(b)) {   // a view that does not start on a 16-byte boundary
        OP_LAUNCH(c, matvec_unaligned, dim3((unsigned)((o_rows + 3) / 4)), dim3(kWG), 0, o, a, b, (int)width, (int)o_rows);
        return 0;
    }
    return counted(c, launch_rows<false, EPI_STORE>(c, o, a, b, nullptr, (int)width, (int)o_rows));
}
int rama_softmax(rama_ctx* c, float* x, size_t n) {
    RAMA_ENTER(c);      // (as rama_sinu)
    REQUIRE(c && x && n > 0, RAMA_EINVAL, "softmax: bad argument");
    RAMA_WRITES(c, x, n);
    if (c->tune_ref_order && c->tune_chain && rmsnorm_chain_ok(n)) return counted(c, launch_softmax_chain(c, x, (int)n));
    if (c->tune_ref_order) { OP_LAUNCH(c, softmax_ref_kernel, dim3(1), dim3(1024), 0, x, (int)n); return 0; }
    OP_LAUNCH(c, softmax_kernel, dim3(1), dim3(1024), 0, x, (int)n);
    return 0;
}

static int attn_nsplit(const rama_ctx* c, int n_heads) {
    if (c->tune_attn_nsplit > 0) return c->tune_attn_nsplit;
    return std::max(1, std::min(16, c->cu_count / std::max(n_heads, 1)));
}

// scratch for the split-T partials; called outside any stream capture (no allocation inside one)
static int ensure_attn_part(rama_ctx* c, const rama_config* cfg) {
    if (set_device(c)) return 1;
    const int hs = cfg->dim / cfg->n_heads;
    const size_t need = (size_t)cfg->n_heads * attn_nsplit(c, cfg->n_heads) * (hs + 4);
    if (need > c->attn_part_floats) {
        if (c->attn_part) { HIPCHK(hipStreamSynchronize(c->stream)); drop_graph(c); HIPCHK(hipFree(c->attn_part)); c->attn_part = nullptr; }      // (graphs captured for a smaller model hold the old address)
        HIPCHK(hipMalloc(&c->attn_part, need * sizeof(float)));
        c->attn_part_floats = need;
    }
    if (c->tune_ref_order) { const int rs = ensure_attn_scores(c, cfg->n_heads, cfg->seq_len); if (rs) return rs; }
    return 0;
}

// Split-T attention is worth its extra (combine) launch once a head's cache no longer fits a
// couple of single-workgroup rounds; below the threshold one workgroup per head is faster.
constexpr int kSplitTPos = 256;
// Measured (tools/split_sweep.py, round 2: 8-wave slices, nt cache loads): at llama2-7B (32 heads x 128)
// splitting wins from ~position 256 on (227 -> 231 tok/s at 300, 217 -> 229 at 600, 183 -> 219 at 1900) and
// loses below it (237 vs 231 at 200); at the stories110M shape (12 heads x 64, 1024
// positions) the single-workgroup kernel wins everywhere (2 837 vs 2 082 tok/s at 900), because
// its whole per-head cache is a few rounds of one workgroup and the combine launch costs more.
static int split_threshold(const rama_ctx* c, const rama_config* cfg) {
    if (c->tune_split_pos >= 0) return c->tune_split_pos;
    const int hs = cfg->dim / cfg->n_heads;
    // a context the one-workgroup kernel's LDS score buffer cannot hold (seq_len > ~15 000) must split
    if (!attn_one_wg_holds(hs, cfg->seq_len)) return kSplitTPos;
    const long kv_bytes_per_pos = 2L * hs * 4;          // one head's K + V row
    return kv_bytes_per_pos * cfg->seq_len <= (1L << 20) ? (1 << 30) : kSplitTPos;   // whole head cache <= 1 MiB: never split
}

// positions up to which the 4-wave attention workgroup is used (it covers 64 timesteps per round;
// measured faster than the 16-wave one up to ~250 timesteps at head sizes 48 / 64)
// Below the split-T threshold an 8-wave workgroup per head covers 128 timesteps per round instead of
// the 16-wave kernel's 256: fewer waves to synchronise, measured +0.7 % tokens/s at llama2-7B for
// positions 8..135 (tools/small_attn_sweep.py).  Not where attention is merged with Wo (dim <= 1024).
static bool merge_wanted(const rama_ctx* c, int dim) { return c->tune_merge < 0 ? dim <= 1024 : c->tune_merge != 0; }
static bool small_attn_at(const rama_ctx* c, int pos, bool split, int dim) {
    if (split || c->tune_small_attn == 0) return false;
    if (c->tune_small_attn == 1) return true;
    return !merge_wanted(c, dim) && pos < c->tune_small_pos;
}

// Which launches a step at `pos` consists of (one hipGraph per variant): fast mode 0 = one 16-wave workgroup per head,
// 1 = split-T (long contexts), 2 = fewer waves per head (short contexts); parity mode 0 = 4 waves per head, 1 = 8 (pos >= 256),
// 2 = launches spread over the chip (pos >= tune_spread_pos); bar mode 0 = parity mode's 4 waves per head below bar_pos_eff, from there on the fast
// mode's variants as 1 = split-T, 2 = fewer waves per head, 3 = one 16-wave workgroup per head
static int bar_pos_eff(const rama_ctx* c) { return std::max(0, std::min(std::min(c->tune_bar_pos, c->tune_spread_pos), kLongAttnPos)); }
static int attn_variant(const rama_ctx* c, const rama_config* cfg, int pos) {
    if (c->tune_ref_order && !c->tune_tol && !(c->tune_bar && pos >= bar_pos_eff(c))) return pos >= c->tune_spread_pos ? 2 : (pos >= kLongAttnPos ? 1 : 0);
    const bool split = pos >= split_threshold(c, cfg);
    const int v = split ? 1 : (small_attn_at(c, pos, split, cfg->dim) ? 2 : 0);
    return (c->tune_ref_order && c->tune_bar && v == 0) ? 3 : v;
}
static int apply_attn_variant(rama_ctx* c, const rama_config* cfg, int pos) {
    c->split_attn = pos >= split_threshold(c, cfg);
    c->small_attn = small_attn_at(c, pos, c->split_attn, cfg->dim);
    c->long_attn = pos >= kLongAttnPos;
    c->spread_attn = pos >= c->tune_spread_pos;
    c->bar_fast = c->tune_ref_order && !c->tune_tol && c->tune_bar && pos >= bar_pos_eff(c);
    return c->variant = attn_variant(c, cfg, pos);
}

static int launch_attention(rama_ctx* c, float* xb, float* att, const float* q, const float* kc_layer,
                            const float* vc_layer, const Ctl* ctl, int pos, int dim, int head_size,
                            int seq_len, int n_heads, bool split = false) {
    REQUIRE(head_size % 4 == 0 && head_size >= 4 && head_size <= 256, RAMA_EUNSUP, "attention: head_size must be a multiple of 4 in [4, 256]");
    REQUIRE(aligned16(q) && aligned16(kc_layer) && aligned16(vc_layer) && aligned16(xb) && dim % 4 == 0, RAMA_EINVAL, "attention: buffers must be 16-byte aligned");
    AttnParams p{};
    p.q = q; p.kc = kc_layer; p.vc = vc_layer; p.att = att; p.xb = xb; p.ctl = ctl; p.pos_val = pos;
    p.dim = dim; p.head_size = head_size; p.seq_len = seq_len;
    const int G = attn_group_width(head_size);
    if (split) {
        const int nsplit = attn_nsplit(c, n_heads);
        REQUIRE((size_t)n_heads * nsplit * (head_size + 4) <= c->attn_part_floats, RAMA_EINVAL, "attention: split-T scratch not prepared");
        p.part = c->attn_part; p.nsplit = nsplit; p.att = nullptr;
        const int chunk_max = (seq_len + nsplit - 1) / nsplit;
        dim3 grid(n_heads, nsplit);
        // template dispatch: G lanes per row x W waves per workgroup x cache-load policy
#define RAMA_SPLIT_LAUNCH(G_, W_, NT_, U_) RAMA_LAUNCH(c, (attention_kernel<G_, true, W_, NT_, U_>), grid, dim3(W_ * 64), (size_t)(attn_scratch_floats(G_, W_) + chunk_max) * sizeof(float), p)
#define RAMA_SPLIT_G(W_, NT_, U_) do { if (G == 16) RAMA_SPLIT_LAUNCH(16, W_, NT_, U_); else if (G == 32) RAMA_SPLIT_LAUNCH(32, W_, NT_, U_); else RAMA_SPLIT_LAUNCH(64, W_, NT_, U_); } while (0)
        const int W = c->tune_attn_waves;
        const bool deep = c->tune_attn_u == 16 && W <= 8;          // 16 rows of K and of V per lane in flight: 128 VGPRs, fine at <= 2 waves per SIMD
        if (c->tune_attn_nt) {
            if (W == 4) { if (deep) RAMA_SPLIT_G(4, true, 16); else RAMA_SPLIT_G(4, true, 8); }
            else if (W == 8) { if (deep) RAMA_SPLIT_G(8, true, 16); else RAMA_SPLIT_G(8, true, 8); }
            else RAMA_SPLIT_G(16, true, 8);
        } else {
            if (W == 4) { if (deep) RAMA_SPLIT_G(4, false, 16); else RAMA_SPLIT_G(4, false, 8); }
            else if (W == 8) { if (deep) RAMA_SPLIT_G(8, false, 16); else RAMA_SPLIT_G(8, false, 8); }
            else RAMA_SPLIT_G(16, false, 8);
        }
#undef RAMA_SPLIT_G
#undef RAMA_SPLIT_LAUNCH
        LAUNCHCHK();
        {
            const dim3 cg(n_heads), cb(((head_size + 63) / 64) * 64);
            const float* part = c->attn_part;
            if (c->tune_combine_v == 0) hipLaunchKernelGGL(attention_combine_loop_kernel, cg, cb, 0, c->stream, part, xb, head_size, nsplit);
            else if (nsplit <= 8) hipLaunchKernelGGL(attention_combine_kernel<8>, cg, cb, 0, c->stream, part, xb, head_size, nsplit);
            else if (nsplit <= 16) hipLaunchKernelGGL(attention_combine_kernel<16>, cg, cb, 0, c->stream, part, xb, head_size, nsplit);
            else hipLaunchKernelGGL(attention_combine_kernel<32>, cg, cb, 0, c->stream, part, xb, head_size, nsplit);
        }
        LAUNCHCHK();
        return 0;
    }
    if (c->small_attn) {     // short contexts: fewer waves per head, one round covers the whole context
        const int W = c->tune_small_waves;
        // score buffer: seq_len timesteps, or what 64 KiB hold when the context is longer (this variant only runs below
        // tune_small_pos, and such models split from position 256 on: split_threshold)
        const int cap4 = std::min(seq_len, (int)(64 * 1024 / sizeof(float)) - attn_scratch_floats(G, W));
        REQUIRE((ctl ? c->host_pos : pos) < cap4, RAMA_EUNSUP, "attention: position beyond the single-workgroup kernel's score buffer");
        size_t shm4 = (size_t)(attn_scratch_floats(G, W) + cap4) * sizeof(float);
#define RAMA_SMALL_G(W_) do { if (G == 16) RAMA_LAUNCH(c, (attention_kernel<16, false, W_>), dim3(n_heads), dim3(W_ * 64), shm4, p); \
                              else if (G == 32) RAMA_LAUNCH(c, (attention_kernel<32, false, W_>), dim3(n_heads), dim3(W_ * 64), shm4, p); \
                              else RAMA_LAUNCH(c, (attention_kernel<64, false, W_>), dim3(n_heads), dim3(W_ * 64), shm4, p); } while (0)
        if (W == 4) RAMA_SMALL_G(4); else RAMA_SMALL_G(8);
#undef RAMA_SMALL_G
        LAUNCHCHK();
        return 0;
    }
    // score buffer: seq_len timesteps, or what 64 KiB hold when the context is longer (such models run
    // split-T from position 256 on, split_threshold; a known position beyond the buffer is an error)
    const int cap = std::min(seq_len, (int)(64 * 1024 / sizeof(float)) - attn_scratch_floats(G));
    REQUIRE((ctl ? c->host_pos : pos) < cap, RAMA_EUNSUP, "attention: position beyond the single-workgroup kernel's score buffer");
    size_t shm = (size_t)(attn_scratch_floats(G) + cap) * sizeof(float);
    if (G == 16) RAMA_LAUNCH(c, (attention_kernel<16, false>), dim3(n_heads), dim3(kAttnThreads), shm, p);
    else if (G == 32) RAMA_LAUNCH(c, (attention_kernel<32, false>), dim3(n_heads), dim3(kAttnThreads), shm, p);
    else RAMA_LAUNCH(c, (attention_kernel<64, false>), dim3(n_heads), dim3(kAttnThreads), shm, p);
    LAUNCHCHK();
    return 0;
}

int rama_multi_head_attention(rama_ctx* c, float* xb, float* att, const float* q, const float* key_cache,
                              const float* value_cache, int layer, int dim, int pos, int head_size,
                              int seq_len, int n_heads) {
    RAMA_ENTER(c);
    REQUIRE(c && xb && att && q && key_cache && value_cache, RAMA_EINVAL, "multi_head_attention: NULL argument");
    REQUIRE(pos >= 0 && pos < seq_len && layer >= 0 && n_heads > 0 && n_heads * head_size == dim, RAMA_EINVAL, "multi_head_attention: bad shape");
    RAMA_WRITES(c, xb, dim); RAMA_WRITES(c, att, (size_t)n_heads * seq_len);
    const size_t lo = (size_t)layer * seq_len * dim;   // cpu.rs:28
    if (c->tune_ref_order && c->tune_bar && !c->tune_tol && pos >= bar_pos_eff(c)) {      // bar mode behind its switch: the fast path's single-workgroup kernel (the 1:1 path prepares no split-T scratch)
        c->small_attn = small_attn_at(c, pos, false, dim);
        return launch_attention(c, xb, att, q, key_cache + lo, value_cache + lo, nullptr, pos, dim, head_size, seq_len, n_heads);
    }
    if (c->tune_ref_order && c->tune_chain && attn_chain_ok(head_size, seq_len) && aligned16(q) && aligned16(key_cache + lo) && aligned16(value_cache + lo) && dim % 4 == 0)
        return launch_attention_chain(c, xb, att, q, key_cache + lo, value_cache + lo, nullptr, pos, dim, head_size, seq_len, n_heads, pos >= kLongAttnPos, pos >= c->tune_spread_pos);
    if (c->tune_ref_order) return launch_attention_ref(c, xb, att, q, key_cache + lo, value_cache + lo, nullptr, pos, dim, head_size, seq_len, n_heads);
    c->small_attn = small_attn_at(c, pos, false, dim);
    return launch_attention(c, xb, att, q, key_cache + lo, value_cache + lo, nullptr, pos, dim, head_size, seq_len, n_heads);
}

int rama_ref_expf(rama_ctx* c, float* o, const float* x, size_t n) {
    RAMA_ENTER(c);
    REQUIRE(c && (n == 0 || (o && x)), RAMA_EINVAL, "ref_expf: NULL argument");
    if (!n) return 0;
    hipLaunchKernelGGL(expf_glibc_kernel, dim3(ew_grid(n)), dim3(256), 0, c->stream, o, x, n);
    LAUNCHCHK(); return 0;
}

// ---------------------------------------------------------------- synthetic fill

int rama_fill_synth(rama_ctx* c, float* dst, size_t n, uint64_t seed, uint64_t tag, uint64_t offset, float scale, float bias) {
    RAMA_ENTER(c);
    REQUIRE(c && (n == 0 || dst), RAMA_EINVAL, "fill_synth: NULL argument");
    RAMA_WRITES(c, dst, n);
    if (!n) return 0;
    const uint64_t base = offset + tag * 0x9E3779B97F4A7C15ULL + seed * 0xD1B54A32D192ED03ULL;
    int grid = (int)std::min<size_t>((n + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(fill_synth_kernel, dim3(grid), dim3(256), 0, c->stream, dst, n, base, scale, bias);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------- fused decode path

int check_cfg(const rama_config* cfg) {
    REQUIRE(cfg, RAMA_EINVAL, "config is NULL");
    REQUIRE(cfg->dim > 0 && cfg->hidden_dim > 0 && cfg->n_layers > 0 && cfg->n_heads > 0 && cfg->vocab_size > 0 && cfg->seq_len > 0, RAMA_EINVAL, "config: non-positive field");
    REQUIRE(cfg->n_kv_heads == cfg->n_heads, RAMA_EUNSUP, "config: n_kv_heads != n_heads (the reference indexes the cache with stride dim, infer.rs:31-33)");
    REQUIRE(cfg->dim % cfg->n_heads == 0, RAMA_EINVAL, "config: dim % n_heads != 0");
    REQUIRE(cfg->dim % 4 == 0 && cfg->hidden_dim % 4 == 0, RAMA_EINVAL, "config: dim and hidden_dim must be multiples of 4 (cpu.rs:142-143)");
    const int hs = cfg->dim / cfg->n_heads;
    REQUIRE(hs % 4 == 0 && hs <= 256, RAMA_EUNSUP, "config: head_size must be a multiple of 4, <= 256");
    return 0;
}

// attention + Wo as one launch (attn_wo.hpp) -- only if the WHOLE grid is resident at
// once according to the occupancy API, which is what makes its in-kernel wait deadlock-free.
// Returns 1 if launched, 0 if the caller must use the two separate launches, < 0 / > 0 on error.
static int try_launch_attn_wo(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                              size_t li, float* kc, float* vc, bool* launched) {
    *launched = false;
    const int dim = cfg->dim, hs = dim / cfg->n_heads;
    const int G = attn_group_width(hs);
    const int gi = G == 16 ? 0 : (G == 32 ? 1 : 2);
    const int grid = (dim + 3) / 4;
    if (cfg->n_heads > grid || !aligned16(s->q) || !aligned16(s->xb) || !aligned16(kc) || !aligned16(vc)) return 0;
    const size_t lds = (size_t)(kPWaves * 4 + p_attn_lds_floats(G, cfg->seq_len)) * sizeof(float);
    if (lds > 64 * 1024) return 0;
    const void* fn = G == 16 ? (const void*)attn_wo_kernel<16> : (G == 32 ? (const void*)attn_wo_kernel<32> : (const void*)attn_wo_kernel<64>);
    if (c->merge_blocks_per_cu[gi] < 0 || c->merge_lds[gi] != lds) {
        int nb = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kPThreads, lds));
        c->merge_blocks_per_cu[gi] = nb; c->merge_lds[gi] = lds;
    }
    // The occupancy API over-reports by one block per CU only for kernels with > 80 SGPRs
    // (MI355X_MICROARCH.md, Residency); this kernel uses 58 (build remark), so its answer is
    // taken as is.  Should the grid not fit, the two separate launches are used instead.
    if ((long)c->merge_blocks_per_cu[gi] * c->cu_count < grid) return 0;
    AttnWoParams a{};
    a.dim = dim; a.n_heads = cfg->n_heads; a.seq_len = cfg->seq_len;
    a.q = s->q; a.kc = kc; a.vc = vc; a.xb = s->xb; a.x = s->x; a.wo = w->wo + li * (size_t)dim * dim;
    a.ctl = c->ctl; a.counter = c->attn_counter; a.err = c->pbar + 1;
    if (G == 16) hipLaunchKernelGGL(attn_wo_kernel<16>, dim3(grid), dim3(kPThreads), lds, c->stream, a);
    else if (G == 32) hipLaunchKernelGGL(attn_wo_kernel<32>, dim3(grid), dim3(kPThreads), lds, c->stream, a);
    else hipLaunchKernelGGL(attn_wo_kernel<64>, dim3(grid), dim3(kPThreads), lds, c->stream, a);
    LAUNCHCHK();
    *launched = true;
    c->handoff_dirty = true;
    return 0;
}

// a whole stage as two launches (layer_fused.hpp): embedding + counter reset, then every layer and the classifier chained by
// arrival counters.  *launched = false: the shape is not one it takes, the caller enqueues the separate launches.
static bool fused_wanted(const rama_ctx* c, int dim) { return c->tune_fused < 0 ? dim <= 1024 : c->tune_fused != 0; }
static int try_launch_fused(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, const rama_stage* st, bool* launched) {
    *launched = false;
    const int dim = cfg->dim, hidden = cfg->hidden_dim, H = cfg->n_heads, hs = dim / H, V = cfg->vocab_size;
    const int nl = st->layer_end - st->layer_begin;
    if (nl <= 0 && (!st->do_cls || st->do_embed)) return 0;
    if (dim > kFusedMaxDim || hidden > kFusedMaxHidden || nl > kFusedMaxLayers || dim % 4 || hidden % 4 || hs % 4 || hs > 256 || cfg->seq_len % 4) return 0;
    const int G = attn_group_width(hs);
    size_t lds = (size_t)fused_lds_floats(G, cfg->seq_len, dim, hidden) * sizeof(float);
    if (lds > 64 * 1024) return 0;
    if (c->tune_fused_solo < 0 ? dim > 512 : c->tune_fused_solo != 0) lds = kFusedSoloLds;
    if ((double)hidden * dim * 4.0 >= 2147483648.0 || (double)V * dim * 4.0 >= 2147483648.0 || (double)cfg->seq_len * dim * 4.0 >= 2147483648.0) return 0;
    if (!aligned16(s->x) || !aligned16(s->q) || !aligned16(s->xb) || !aligned16(s->hb) || !aligned16(s->key_cache) || !aligned16(s->value_cache) ||
        !aligned16(w->wq) || !aligned16(w->wk) || !aligned16(w->wv) || !aligned16(w->wo) || !aligned16(w->w1) || !aligned16(w->w2) || !aligned16(w->w3) ||
        !aligned16(w->wcls) || !aligned16(w->rms_att_weight) || !aligned16(w->rms_ffn_weight) || !aligned16(w->rms_final_weight)) return 0;
    auto wgs = [](int units) { return (units + kPWaves - 1) / kPWaves; };
    FusedParams a{};
    a.dim = dim; a.hidden = hidden; a.n_heads = H; a.seq_len = cfg->seq_len; a.vocab = V; a.n_layers = nl; a.do_cls = st->do_cls ? 1 : 0;
    a.wq = w->wq; a.wk = w->wk; a.wv = w->wv; a.wo = w->wo; a.w1 = w->w1; a.w3 = w->w3; a.w2 = w->w2;
    a.g_att = w->rms_att_weight; a.g_ffn = w->rms_ffn_weight; a.g_final = w->rms_final_weight; a.wcls = w->wcls;
    a.emb = st->do_embed ? w->token_embedding_table : nullptr;
    a.x = s->x; a.q = s->q; a.k = s->k; a.v = s->v; a.xb = s->xb; a.hb = s->hb; a.logits = s->logits;
    a.kc = s->key_cache; a.vc = s->value_cache; a.fr = w->freq_cis_real; a.fi = w->freq_cis_imag;
    a.ctl = c->ctl; a.hand = c->fused_hand; a.epoch = c->fused_epoch; a.err = c->pbar + 1;
    const bool wide = hidden > 1024;             // W2 units: 2 rows x 8 chunks ahead instead of 4 x 4
    a.nA = wgs(3 * ((dim + 3) / 4)); a.nC = wgs((dim + 3) / 4); a.nD = wgs((hidden + 1) / 2); a.nE = wide ? wgs((dim + 1) / 2) : a.nC;
    const bool cd2 = dim <= 512;
    const long grid = (long)nl * (a.nA + H + a.nC + a.nD + a.nE) + (st->do_cls ? (cd2 ? wgs((V + 7) / 8) : wgs((V + 3) / 4)) : 0);
#define RAMA_FUSED_(G_, CD_) do { if (wide) hipLaunchKernelGGL((stage_fused_kernel<G_, CD_, 2, 8>), dim3((unsigned)grid), dim3(kPThreads), lds, c->stream, a); \
                                  else hipLaunchKernelGGL((stage_fused_kernel<G_, CD_, 4, 4>), dim3((unsigned)grid), dim3(kPThreads), lds, c->stream, a); } while (0)
#define RAMA_FUSED(G_, CD_) RAMA_FUSED_(G_, CD_)
    if (G == 16) { if (cd2) RAMA_FUSED(16, 2); else RAMA_FUSED(16, 4); }
    else if (G == 32) { if (cd2) RAMA_FUSED(32, 2); else RAMA_FUSED(32, 4); }
    else { if (cd2) RAMA_FUSED(64, 2); else RAMA_FUSED(64, 4); }
#undef RAMA_FUSED_
#undef RAMA_FUSED
    LAUNCHCHK();
    *launched = true;
    c->handoff_dirty = true;
    if (c->fused_chained) { c->fused_epoch_owed = true; return 0; }      // the sampler that follows advances the epoch
    hipLaunchKernelGGL(fused_epoch_kernel, dim3(1), dim3(1), 0, c->stream, c->fused_epoch);
    LAUNCHCHK();
    return 0;
}

// the fast path's norm-folding launches of a layer (also what tolerance mode's "tol_mask" swaps in for A/B runs)
// infer.rs:19-33: rmsnorm, Wq|Wk|Wv, RoPE, cache append
static int launch_fast_qkv(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, size_t li, float* kc, float* vc) {
    const int dim = cfg->dim, hs = dim / cfg->n_heads;
    const size_t dd = (size_t)dim * dim;
    KTimer kt(c, RAMA_K_QKV);
    GemvParams p{};
    p.w[0] = w->wq + li * dd; p.w[1] = w->wk + li * dd; p.w[2] = w->wv + li * dd;
    p.x = s->x; p.nw = w->rms_att_weight + li * dim;
    p.o[0] = s->q; p.o[1] = s->k; p.o[2] = s->v;
    p.K = dim; p.rows = dim; p.nmat = 3;
    p.ctl = c->ctl; p.fr = w->freq_cis_real; p.fi = w->freq_cis_imag; p.head_size = hs;
    p.kc = kc; p.vc = vc;
    p.zero_me = c->attn_counter;
    if (use_solo(c, dim)) {
        const dim3 grid((3 * ((dim + 3) / 4) + kSoloWaves - 1) / kSoloWaves), block(kSoloWaves * 64);
        if (dim <= 512) RAMA_LAUNCH(c, (gemv_rows_solo<4, 2, true, EPI_QKV>), grid, block, 0, p);
        else RAMA_LAUNCH(c, (gemv_rows_solo<4, 4, true, EPI_QKV>), grid, block, 0, p);
    } else {
        DISPATCH_GEOM(c, RAMA_LAUNCH(c, (gemv_rows<R_, CH_, NW_, true, EPI_QKV>), dim3(3 * (dim / R_)), dim3(NW_ * 64), 0, p));
    }
    LAUNCHCHK();
    return 0;
}
// infer.rs:39-45: rmsnorm, W1|W3, SiLU * gate (w13i: the model's row-interleaved copy, or NULL)
static int launch_fast_w13(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, size_t li, const float* w13i) {
    const int dim = cfg->dim, hidden = cfg->hidden_dim;
    const size_t hd = (size_t)hidden * dim;
    KTimer kt(c, RAMA_K_W13);
    if (w13i && c->tune_w13i) {
        // the model's row-interleaved copy: one [2 hidden, dim] matrix, rows (2i, 2i + 1) = (W1 row i, W3 row i)
        GemvParams p{};
        p.w[0] = w13i + li * 2 * hd; p.x = s->x; p.nw = w->rms_ffn_weight + li * dim; p.o[0] = s->hb;
        p.K = dim; p.rows = 2 * hidden; p.nmat = 1;
        if (use_solo(c, dim)) {
            const dim3 grid(((2 * hidden + 3) / 4 + kSoloWaves - 1) / kSoloWaves), block(kSoloWaves * 64);
            if (dim <= 512) RAMA_LAUNCH(c, (gemv_rows_solo<4, 2, true, EPI_SWIGLU_PAIR>), grid, block, 0, p);
            else RAMA_LAUNCH(c, (gemv_rows_solo<4, 4, true, EPI_SWIGLU_PAIR>), grid, block, 0, p);
        } else {
            RAMA_LAUNCH(c, (gemv_rows<4, 2, 8, true, EPI_SWIGLU_PAIR>), dim3((2 * hidden + 3) / 4), dim3(8 * 64), 0, p);
        }
    } else {
        SwigluParams p{};
        p.w1 = w->w1 + li * hd; p.w3 = w->w3 + li * hd; p.x = s->x; p.nw = w->rms_ffn_weight + li * dim;
        p.hb = s->hb; p.K = dim; p.rows = hidden;
        if (use_solo(c, dim)) {
            const dim3 grid(((hidden + 1) / 2 + kSoloWaves - 1) / kSoloWaves), block(kSoloWaves * 64);
            if (dim <= 512) RAMA_LAUNCH(c, (gemv_swiglu_solo<2, 2>), grid, block, 0, p);
            else RAMA_LAUNCH(c, (gemv_swiglu_solo<2, 4>), grid, block, 0, p);
        } else {
            DISPATCH_GEOM(c, RAMA_LAUNCH(c, (gemv_swiglu<R2_, CH_, NW_>), dim3((hidden + R2_ - 1) / R2_), dim3(NW_ * 64), 0, p));
        }
    }
    LAUNCHCHK();
    return 0;
}

// infer.rs:8-53 op by op in the reference's rounding order (ref_order.hpp); leaves EVERY RunState
// buffer as the CPU path does (x, xb, xb2, hb, hb2, q, k, v, att, logits, caches)
static int enqueue_stage_ref(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, const rama_stage* st) {
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads;
    const size_t dd = (size_t)dim * dim, hd = (size_t)hidden * dim;
    int rc;
    REQUIRE(s->xb2 && s->hb2 && s->k && s->v, RAMA_EINVAL, "forward (reference order): xb2 / hb2 / k / v buffers are required");
    if (st->do_embed) {
        hipLaunchKernelGGL(embed_kernel, dim3((dim + 255) / 256), dim3(256), 0, c->stream, s->x, w->token_embedding_table, (const Ctl*)c->ctl, 0, dim);
        LAUNCHCHK();
    }
    for (int layer = st->layer_begin; layer < st->layer_end; layer++) {
        const size_t li = (size_t)(layer - st->layer_begin);
        float* kc = s->key_cache + li * cfg->seq_len * dim;
        float* vc = s->value_cache + li * cfg->seq_len * dim;
        rc = launch_rmsnorm_ref(c, s->xb, s->x, w->rms_att_weight + li * dim, dim); if (rc) return rc;          // infer.rs:19
        {   // :20-23
            float* const oo[3] = {s->q, s->k, s->v};
            const float* const ww[3] = {w->wq + li * dd, w->wk + li * dd, w->wv + li * dd};
            rc = launch_matvec_ref(c, 3, oo, ww, s->xb, dim, dim); if (rc) return rc;
        }
        hipLaunchKernelGGL(rope_ref_cursor_kernel, dim3((dim / 2 + 255) / 256), dim3(256), 0, c->stream, s->q, s->k, (const float*)s->v,
                           w->freq_cis_real, w->freq_cis_imag, dim, hs, kc, vc, (const Ctl*)c->ctl);                                // :25-33
        LAUNCHCHK();
        rc = launch_attention_ref(c, s->xb, s->att, s->q, kc, vc, c->ctl, 0, dim, hs, cfg->seq_len, cfg->n_heads); if (rc) return rc;   // :34
        rc = launch_matvec_ref1(c, s->xb2, w->wo + li * dd, s->xb, dim, dim); if (rc) return rc;                  // :35
        hipLaunchKernelGGL(array_add_kernel, dim3(ew_grid(dim)), dim3(256), 0, c->stream, s->x, (const float*)s->xb2, (size_t)dim);   // :37
        LAUNCHCHK();
        rc = launch_rmsnorm_ref(c, s->xb, s->x, w->rms_ffn_weight + li * dim, dim); if (rc) return rc;            // :39
        {   // :41-42
            float* const oo[3] = {s->hb, s->hb2, nullptr};
            const float* const ww[3] = {w->w1 + li * hd, w->w3 + li * hd, nullptr};
            rc = launch_matvec_ref(c, 2, oo, ww, s->xb, dim, hidden); if (rc) return rc;
        }
        hipLaunchKernelGGL(sinu_ref_kernel, dim3(ew_grid(hidden)), dim3(256), 0, c->stream, s->hb, (size_t)hidden);                  // :44
        LAUNCHCHK();
        hipLaunchKernelGGL(array_mult_kernel, dim3(ew_grid(hidden)), dim3(256), 0, c->stream, s->hb, (const float*)s->hb2, (size_t)hidden);   // :45
        LAUNCHCHK();
        rc = launch_matvec_ref1(c, s->xb, w->w2 + li * hd, s->hb, hidden, dim); if (rc) return rc;                // :46
        hipLaunchKernelGGL(array_add_kernel, dim3(ew_grid(dim)), dim3(256), 0, c->stream, s->x, (const float*)s->xb, (size_t)dim);    // :47
        LAUNCHCHK();
    }
    if (st->do_cls) {
        hipLaunchKernelGGL(copy_kernel, dim3(ew_grid(dim)), dim3(256), 0, c->stream, s->xb, (const float*)s->x, (size_t)dim);         // :49
        LAUNCHCHK();
        rc = launch_rmsnorm_ref(c, s->x, s->xb, w->rms_final_weight, dim); if (rc) return rc;                     // :50
        rc = launch_matvec_ref1(c, s->logits, w->wcls, s->x, dim, cfg->vocab_size); if (rc) return rc;            // :51
    }
    return 0;
}

// the same (every RunState buffer as the CPU path leaves it, bit for bit) on the model's chain-order weight
// copies: 7 launches per layer.  Returns false when a copy is missing (weights uploaded tensor by tensor,
// widths that are not whole 16-float blocks, no memory for the copy): the caller takes enqueue_stage_ref.
static int enqueue_stage_chain(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, const rama_stage* st, bool* done) {
    *done = false;
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads, V = cfg->vocab_size;
    if (!c->tune_chain || dim % 16 || hidden % 16 || dim > 16000 || hidden > 16000 || !attn_chain_ok(hs, cfg->seq_len)) return 0;
    const bool layers = st->layer_end > st->layer_begin;
    const float *cq = nullptr, *ck = nullptr, *cv = nullptr, *co = nullptr, *c13 = nullptr, *c2 = nullptr, *ccls = nullptr;
    if (layers) {
        cq = rama_internal_chain_lookup(w->wq, dim, dim); ck = rama_internal_chain_lookup(w->wk, dim, dim);
        cv = rama_internal_chain_lookup(w->wv, dim, dim); co = rama_internal_chain_lookup(w->wo, dim, dim);
        c13 = rama_internal_chain_lookup(w->w1, 2 * hidden, dim); c2 = rama_internal_chain_lookup(w->w2, dim, hidden);
        if (!cq || !ck || !cv || !co || !c13 || !c2) return 0;
    }
    if (st->do_cls) { ccls = rama_internal_chain_lookup(w->wcls, V, dim); if (!ccls) return 0; }
    REQUIRE(s->xb2 && s->hb2 && s->k && s->v, RAMA_EINVAL, "forward (reference order): xb2 / hb2 / k / v buffers are required");
    *done = true;
    const size_t dd = (size_t)dim * dim, hd = (size_t)hidden * dim;                 // chain-order copies keep the row-major sizes (rows are multiples of 16)
    // tolerance mode ("ref_order" = 2): the matvecs as in parity mode, the norms folded into them as tree-shaped sums (dim <= 8192: all of x
    // in a workgroup's registers; wider models keep the exact-sum norm launches), the fast path's attention
    // "tol_mask" (A/B runs that say which op carries how much of the distance to the CPU path): 1 / 2 / 4 / 8 / 16 = the fast path's
    // Wq|Wk|Wv / Wo / W1|W3 / W2 / classifier launch instead of the chain-order one, 32 = parity mode's attention, 64 = its exact-sum norm launches
    const bool tol = c->tune_tol != 0;
    const int mask = tol ? c->tune_tol_mask : 0;
    const bool tol_fold = tol && dim <= 8192 && c->tune_chain_d <= 0 && !(mask & 64);
    // parity mode, narrow models: the exact norms ride in the matvecs that consume them ("chain_norm"; measured: stories15M +6.6 %; at dim
    // 768 the ripples cost more than the launch, -4 %)
    const int par_norm = (!tol && c->tune_chain_d <= 0 && c->tune_chain_norm && dim <= 512) ? CNORM_EXACT : CNORM_NONE;
    // parity mode, wider models ([r5]): the exact sum by a leader workgroup inside the consuming launch ("chain_lead"; x of <= 4096 floats per wave of the
    // matvec's workgroups, layer ranges of <= 256 layers)
    const bool lead_ok = !tol && par_norm == CNORM_NONE && c->tune_chain_lead && c->tune_chain_d <= 0 && dim % 8 == 0 && dim <= 4096 && dim / 16 > 32 &&
                         st->layer_end - st->layer_begin <= 256;      // (per-class timing keeps it: the `norm` class is then the final norm's launch alone, as in the timed step)
    const int lnorm = tol ? (tol_fold ? CNORM_TREE : CNORM_NONE) : (lead_ok ? CNORM_LEAD : par_norm);      // how the layer norms are folded
    bool led = false;
    const float* w13i = (tol && (mask & 4) && st->layer_end > st->layer_begin && (double)hidden * dim * 8.0 < 2147483648.0) ? rama_internal_w13_lookup(w->w1, w->w3) : nullptr;
    int rc;
    if (st->do_embed) {
        hipLaunchKernelGGL(embed_kernel, dim3((dim + 255) / 256), dim3(256), 0, c->stream, s->x, w->token_embedding_table, (const Ctl*)c->ctl, 0, dim);
        LAUNCHCHK();
    }
    for (int layer = st->layer_begin; layer < st->layer_end; layer++) {
        const size_t li = (size_t)(layer - st->layer_begin);
        float* kc = s->key_cache + li * cfg->seq_len * dim;
        float* vc = s->value_cache + li * cfg->seq_len * dim;
        // narrow models: the two norms of a layer ride in the matvecs that consume them (2 of 7 launches; "chain_norm")
        const bool fold = lnorm != CNORM_NONE;
        if (!fold && !(mask & 1)) { KTimer kt(c, RAMA_K_NORM); rc = launch_rmsnorm_chain(c, s->xb, s->x, w->rms_att_weight + li * dim, dim, nullptr); if (rc) return rc; }      // infer.rs:19
        if (mask & 1) { rc = launch_fast_qkv(c, cfg, w, s, li, kc, vc); if (rc) return rc; }
        else {   // :20-33: Wq | Wk | Wv, RoPE, cache append
            KTimer kt(c, RAMA_K_QKV);
            ChainParams p{};
            p.w[0] = cq + li * dd; p.w[1] = ck + li * dd; p.w[2] = cv + li * dd;
            p.o[0] = s->q; p.o[1] = s->k; p.o[2] = s->v; p.x = fold ? s->x : s->xb; p.nw = fold ? w->rms_att_weight + li * dim : nullptr;
            p.K = dim; p.rows = dim; p.nmat = 3;
            p.ctl = c->ctl; p.fr = w->freq_cis_real; p.fi = w->freq_cis_imag; p.head_size = hs; p.kc = kc; p.vc = vc;
            if (lnorm == CNORM_LEAD) { p.lead = c->lead_slots + 32 * (2 * li); p.epoch = c->fused_epoch; p.err = c->pbar + 1; led = true; }
            rc = launch_chain(c, p, CEPI_QKV, fold ? lnorm : CNORM_NONE); if (rc) return rc;
        }
        {   // :34
            KTimer kt(c, RAMA_K_ATTN);
            if ((tol && !(mask & 32)) || c->bar_fast) rc = launch_attention(c, s->xb, s->att, s->q, kc, vc, c->ctl, 0, dim, hs, cfg->seq_len, cfg->n_heads, c->split_attn);
            else rc = launch_attention_chain(c, s->xb, s->att, s->q, kc, vc, c->ctl, 0, dim, hs, cfg->seq_len, cfg->n_heads, c->long_attn, c->spread_attn);
            if (rc) return rc;
        }
        if (mask & 2) { KTimer kt(c, RAMA_K_WO); rc = launch_rows<false, EPI_RESID>(c, s->x, w->wo + li * dd, s->xb, nullptr, dim, dim); if (rc) return rc; }
        else {   // :35-37: xb2 = Wo . xb; x += xb2
            KTimer kt(c, RAMA_K_WO);
            ChainParams p{};
            p.w[0] = co + li * dd; p.o[0] = s->xb2; p.resid = s->x; p.x = s->xb; p.K = dim; p.rows = dim; p.nmat = 1;
            rc = launch_chain(c, p, CEPI_RESID); if (rc) return rc;
        }
        if (!fold && !(mask & 4)) { KTimer kt(c, RAMA_K_NORM); rc = launch_rmsnorm_chain(c, s->xb, s->x, w->rms_ffn_weight + li * dim, dim, nullptr); if (rc) return rc; }       // :39
        if (mask & 4) { rc = launch_fast_w13(c, cfg, w, s, li, w13i); if (rc) return rc; }
        else {   // :41-45: hb = silu(W1 . xb) * (hb2 = W3 . xb)
            KTimer kt(c, RAMA_K_W13);
            ChainParams p{};
            p.w[0] = c13 + li * 2 * hd; p.o[0] = s->hb; p.o[1] = s->hb2; p.x = fold ? s->x : s->xb; p.nw = fold ? w->rms_ffn_weight + li * dim : nullptr;
            p.K = dim; p.rows = 2 * hidden; p.nmat = 1;
            if (lnorm == CNORM_LEAD) { p.lead = c->lead_slots + 32 * (2 * li + 1); p.epoch = c->fused_epoch; p.err = c->pbar + 1; led = true; }
            rc = launch_chain(c, p, CEPI_SWIGLU, fold ? lnorm : CNORM_NONE); if (rc) return rc;
        }
        if (mask & 8) { KTimer kt(c, RAMA_K_W2); rc = launch_rows<false, EPI_RESID>(c, s->x, w->w2 + li * hd, s->hb, nullptr, hidden, dim); if (rc) return rc; }
        else {   // :46-47: xb = W2 . hb; x += xb
            KTimer kt(c, RAMA_K_W2);
            ChainParams p{};
            p.w[0] = c2 + li * hd; p.o[0] = s->xb; p.resid = s->x; p.x = s->hb; p.K = hidden; p.rows = dim; p.nmat = 1;
            rc = launch_chain(c, p, CEPI_RESID); if (rc) return rc;
        }
    }
    if (st->do_cls) {   // :49-51: xb = x; x = rmsnorm(xb); logits = Wcls . x
        // (tolerance mode with the norm folded into the classifier leaves x and xb as the fast path does: the residual stream,
        // not its normalised copy)
        if (mask & 16) { KTimer kt(c, RAMA_K_CLS); return launch_rows<true, EPI_STORE>(c, s->logits, w->wcls, s->x, w->rms_final_weight, dim, V); }
        if (!tol_fold) { KTimer kt(c, RAMA_K_NORM); rc = launch_rmsnorm_chain(c, s->x, s->x, w->rms_final_weight, dim, s->xb); if (rc) return rc; }
        KTimer kt(c, RAMA_K_CLS);
        ChainParams p{};
        p.w[0] = ccls; p.o[0] = s->logits; p.x = s->x; p.K = dim; p.rows = V; p.nmat = 1;
        if (tol_fold) p.nw = w->rms_final_weight;
        rc = launch_chain(c, p, CEPI_STORE, tol_fold ? CNORM_TREE : CNORM_NONE); if (rc) return rc;
    }
    if (led) {      // the leaders' words carry the epoch: it advances after every stage that used them (layer_fused.hpp's convention)
        if (c->fused_chained) c->fused_epoch_owed = true;      // the sampler that follows advances it
        else { hipLaunchKernelGGL(fused_epoch_kernel, dim3(1), dim3(1), 0, c->stream, c->fused_epoch); LAUNCHCHK(); }
    }
    return 0;
}

// one (token, pos) step over a layer range; ctl on the device holds token/pos
static int enqueue_stage(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                         const rama_stage* st) {
    if (c->tune_ref_order) {
        bool done = false;
        const int rc = enqueue_stage_chain(c, cfg, w, s, st, &done);
        return done ? rc : (rc ? rc : enqueue_stage_ref(c, cfg, w, s, st));
    }
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads;
    const size_t dd = (size_t)dim * dim, hd = (size_t)hidden * dim;
    if (fused_wanted(c, dim) && !c->split_attn && !c->small_attn && c->kp.kernel_id < 0) {
        bool launched = false;
        const int rc = try_launch_fused(c, cfg, w, s, st, &launched);
        if (rc || launched) return rc;
    }
    const float* w13i = (st->layer_end > st->layer_begin && (double)hidden * dim * 8.0 < 2147483648.0) ? rama_internal_w13_lookup(w->w1, w->w3) : nullptr;
    if (st->do_embed) {
        hipLaunchKernelGGL(embed_kernel, dim3((dim + 255) / 256), dim3(256), 0, c->stream, s->x, w->token_embedding_table, (const Ctl*)c->ctl, 0, dim);
        LAUNCHCHK();
    }
    for (int layer = st->layer_begin; layer < st->layer_end; layer++) {
        const size_t li = (size_t)(layer - st->layer_begin);
        float* kc = s->key_cache + li * cfg->seq_len * dim;
        float* vc = s->value_cache + li * cfg->seq_len * dim;
        { const int rcq = launch_fast_qkv(c, cfg, w, s, li, kc, vc); if (rcq) return rcq; }      // infer.rs:19-33
        bool merged = false;
        const bool want_merge = merge_wanted(c, dim);
        if (want_merge && !c->split_attn && !c->small_attn && c->kp.kernel_id < 0) {   // infer.rs:34-37 as one launch (per-kernel timing keeps them apart)
            int rc = try_launch_attn_wo(c, cfg, w, s, li, kc, vc, &merged);
            if (rc) return rc;
        }
        if (!merged) {
            {   // infer.rs:34
                KTimer kt(c, RAMA_K_ATTN);
                int rc = launch_attention(c, s->xb, s->att, s->q, kc, vc, c->ctl, 0, dim, hs, cfg->seq_len, cfg->n_heads, c->split_attn);
                if (rc) return rc;
            }
            {   // infer.rs:35-37: x += Wo . xb
                KTimer kt(c, RAMA_K_WO);
                int rc = launch_rows<false, EPI_RESID>(c, s->x, w->wo + li * dd, s->xb, nullptr, dim, dim);
                if (rc) return rc;
            }
        }
        { const int rcw = launch_fast_w13(c, cfg, w, s, li, w13i); if (rcw) return rcw; }        // infer.rs:39-45
        {   // infer.rs:46-47: x += W2 . hb
            KTimer kt(c, RAMA_K_W2);
            int rc = launch_rows<false, EPI_RESID>(c, s->x, w->w2 + li * hd, s->hb, nullptr, hidden, dim);
            if (rc) return rc;
        }
    }
    if (st->do_cls) {   // infer.rs:49-51
        KTimer kt(c, RAMA_K_CLS);
        int rc = launch_rows<true, EPI_STORE>(c, s->logits, w->wcls, s->x, w->rms_final_weight, dim, cfg->vocab_size);
        if (rc) return rc;
    }
    return 0;
}

static bool same_capture(const GraphCache& g, const rama_config* cfg, const rama_weights* w, const rama_run_state* s);

// enqueue_stage, replayed from a hipGraph when graph mode is on: token and position live in the device
// cursor (written by the caller just before), so the launches of a (state, stage, attention variant)
// are the same every time.  Used by rama_forward / rama_forward_stage* -- the per-token entry points
// of a trait-level host and of the pipeline stages (csrc/pipe.hip).
constexpr size_t kMaxStageGraphs = 48;
static int run_stage(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, const rama_stage* st) {
    if (!c->graph_mode || c->kp.kernel_id >= 0) return enqueue_stage(c, cfg, w, s, st);
    const int variant = c->variant;
    rama_ctx::StageGraph* hit = nullptr;
    for (auto& e : c->sg)
        if (e.variant == variant && !memcmp(&e.st, st, sizeof *st) && same_capture(e.g, cfg, w, s)) { hit = &e; break; }
    if (!hit) {
        if (c->sg.size() >= kMaxStageGraphs) {       // evict the entry used longest ago
            size_t old = 0;
            for (size_t i = 1; i < c->sg.size(); i++) if (c->sg[i].used < c->sg[old].used) old = i;
            HIPCHK(hipStreamSynchronize(c->stream));
            destroy_graph(c->sg[old].g.cg);
            c->sg.erase(c->sg.begin() + (long)old);
        }
        rama_ctx::StageGraph e;
        const int rc = capture_graph(c, e.g.cg, [&] { return enqueue_stage(c, cfg, w, s, st); });
        if (rc) return rc;
        e.g.cfg = *cfg; e.g.w = *w; e.g.s = *s; e.g.valid = true; e.g.copies_gen = rama_internal_copies_generation(); e.st = *st; e.variant = variant;
        c->sg.push_back(e);
        hit = &c->sg.back();
    }
    hit->used = ++c->sg_clock;
    return replay_graph(c, hit->g.cg);
}

int check_stage(const rama_config* cfg, const rama_weights* w, const rama_run_state* s, const rama_stage* st) {
    REQUIRE(w && s && st, RAMA_EINVAL, "forward: NULL argument");
    REQUIRE(st->layer_begin >= 0 && st->layer_begin <= st->layer_end && st->layer_end <= cfg->n_layers, RAMA_EINVAL, "forward: bad layer range");
    REQUIRE(cfg->dim % 4 == 0, RAMA_EINVAL, "forward: dim % 4 != 0");
    if (st->layer_end > st->layer_begin)
        REQUIRE(w->wq && w->wk && w->wv && w->wo && w->w1 && w->w2 && w->w3 && w->rms_att_weight && w->rms_ffn_weight && w->freq_cis_real && w->freq_cis_imag, RAMA_EINVAL, "forward: missing layer weights");
    if (st->do_embed) REQUIRE(w->token_embedding_table, RAMA_EINVAL, "forward: missing embedding table");
    if (st->do_cls) REQUIRE(w->wcls && w->rms_final_weight && s->logits, RAMA_EINVAL, "forward: missing classifier weights");
    REQUIRE(s->x && s->xb && s->hb && s->q && s->k && s->v && s->att && s->key_cache && s->value_cache, RAMA_EINVAL, "forward: missing state buffer");
    return 0;
}

// parity mode's chain-order weight copy: made on first use for a resident model -- and for weights that were uploaded tensor by tensor (hbm.rs:55-90),
// which are adopted first (model.hip rama_internal_adopt): the reference's own upload path then runs the same kernels as rama_model_load
int ensure_chain_copy(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_stage* st) {
    const rama_stage full{0, cfg->n_layers, 1, 1};
    const int rc = rama_internal_adopt(c, cfg, st ? st : &full, w);
    return rc ? rc : rama_internal_model_ensure(c, w, 1);
}

int rama_forward_stage(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                       int token, int pos, const rama_stage* st) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    if (set_device(c)) return 1;
    int rc = check_cfg(cfg); if (rc) return rc;
    rc = check_stage(cfg, w, s, st); if (rc) return rc;
    REQUIRE(pos >= 0 && pos < cfg->seq_len, RAMA_EINVAL, "forward: pos outside [0, seq_len)");
    REQUIRE(token >= 0 && token < cfg->vocab_size, RAMA_EINVAL, "forward: token outside the vocabulary");
    rc = ensure_attn_part(c, cfg); if (rc) return rc;
    if (c->tune_ref_order && c->tune_chain) { rc = ensure_chain_copy(c, cfg, w, st); if (rc) return rc; }
    hipLaunchKernelGGL(set_ctl_kernel, dim3(1), dim3(1), 0, c->stream, c->ctl, token, pos, 0, 0);
    LAUNCHCHK();
    c->embedded_x = nullptr;
    c->host_pos = -1;
    apply_attn_variant(c, cfg, pos);
    return run_stage(c, cfg, w, s, st);
}

// pipeline-stage variants: the token id stays in device memory end to end
int rama_forward_stage_devtok(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                              const int32_t* token_dev, int pos, const rama_stage* st) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    if (set_device(c)) return 1;
    int rc = check_cfg(cfg); if (rc) return rc;
    rc = check_stage(cfg, w, s, st); if (rc) return rc;
    REQUIRE(pos >= 0 && pos < cfg->seq_len, RAMA_EINVAL, "forward: pos outside [0, seq_len)");
    REQUIRE(token_dev || !st->do_embed, RAMA_EINVAL, "forward: an embedding stage needs a token");
    rc = ensure_attn_part(c, cfg); if (rc) return rc;
    if (c->tune_ref_order && c->tune_chain) { rc = ensure_chain_copy(c, cfg, w, st); if (rc) return rc; }
    hipLaunchKernelGGL(set_ctl_dev_kernel, dim3(1), dim3(1), 0, c->stream, c->ctl, (const int*)token_dev, pos, cfg->vocab_size);
    LAUNCHCHK();
    c->embedded_x = nullptr;
    c->host_pos = -1;
    apply_attn_variant(c, cfg, pos);
    return run_stage(c, cfg, w, s, st);
}

int rama_forward(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, int token, int pos) {
    RAMA_ENTER(c);
    REQUIRE(cfg, RAMA_EINVAL, "config is NULL");
    rama_stage st{0, cfg->n_layers, 1, 1};
    return rama_forward_stage(c, cfg, w, s, token, pos, &st);
}

// ---- device-chained greedy decode (generate() at T == 0, mod.rs:169-206)

// a new generation: nothing of the old one may still be on its way to the ring, then the used part is cleared
static int ring_reset(rama_ctx* c) {
    if (c->ring_hi > 0) {
        HIPCHK(hipStreamSynchronize(c->stream));
        memset(c->ring, 0, sizeof(int) * (size_t)std::min(c->ring_hi, c->out_cap));
        c->ring_hi = 0;
    }
    return 0;
}

int rama_decode_begin(rama_ctx* c, int token, int pos, const int32_t* forced_host, int n_forced) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    { int rr = ring_reset(c); if (rr) return rr; }
    REQUIRE(n_forced >= 0 && n_forced <= c->forced_cap, RAMA_EINVAL, "decode_begin: too many forced tokens");
    REQUIRE(n_forced == 0 || forced_host, RAMA_EINVAL, "decode_begin: forced list is NULL");
    if (n_forced) {
        HIPCHK(hipMemcpyAsync(c->forced, forced_host, sizeof(int) * n_forced, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    hipLaunchKernelGGL(set_ctl_kernel, dim3(1), dim3(1), 0, c->stream, c->ctl, token, pos, n_forced, 0);
    LAUNCHCHK();
    c->embedded_x = nullptr;   // the first decode step must gather x = emb[token] itself
    c->host_pos = pos;         // the chained loop advances pos by one per step: the host can mirror it
    return 0;
}

// One chained step: layers + classifier + (argmax, cursor advance, next token's embedding
// gather).  x already holds emb[token] on entry (rama_decode_steps primes it once).
static int enqueue_decode_step(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s) {
    rama_stage st{0, cfg->n_layers, 0, 1};
    c->fused_chained = true; c->fused_epoch_owed = false;
    int rc = enqueue_stage(c, cfg, w, s, &st);
    c->fused_chained = false;
    if (rc) return rc;
    ArgmaxParams ap{};
    ap.logits = s->logits; ap.n = cfg->vocab_size;
    ap.ctl = c->ctl; ap.forced = c->forced; ap.out = c->out; ap.out_cap = c->out_cap; ap.ring = c->ring_dev;
    ap.emb = w->token_embedding_table; ap.x = s->x; ap.dim = cfg->dim;
    if (c->fused_epoch_owed) ap.epoch = c->fused_epoch;
    rc = enqueue_sample(c, ap, c->samp_T, c->samp_topp, c->samp_u);
    if (rc && c->fused_epoch_owed) {      // the stage launch is enqueued and counted on the sampler to advance the epoch: do it here, or the next
        hipLaunchKernelGGL(fused_epoch_kernel, dim3(1), dim3(1), 0, c->stream, c->fused_epoch);      // launch would take this one's tagged vectors for its own
        (void)hipGetLastError();
    }
    c->fused_epoch_owed = false;
    return rc;
}

static bool same_capture(const GraphCache& g, const rama_config* cfg, const rama_weights* w, const rama_run_state* s) {
    return g.valid && g.copies_gen == rama_internal_copies_generation() && !memcmp(&g.cfg, cfg, sizeof *cfg) && !memcmp(&g.w, w, sizeof *w) && !memcmp(&g.s, s, sizeof *s);
}

int rama_decode_steps(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s, int n_steps) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    if (set_device(c)) return 1;
    int rc = check_cfg(cfg); if (rc) return rc;
    rama_stage st{0, cfg->n_layers, 1, 1};
    rc = check_stage(cfg, w, s, &st); if (rc) return rc;
    REQUIRE(n_steps >= 0, RAMA_EINVAL, "decode_steps: n_steps < 0");
    if (n_steps == 0) return 0;
    if (c->embedded_x != s->x) {   // infer.rs:13 for the first step; later steps get it from the argmax kernel
        hipLaunchKernelGGL(embed_kernel, dim3((cfg->dim + 255) / 256), dim3(256), 0, c->stream, s->x, w->token_embedding_table, (const Ctl*)c->ctl, 0, cfg->dim);
        LAUNCHCHK();
        c->embedded_x = s->x;
    }
    REQUIRE(c->host_pos >= 0, RAMA_EINVAL, "decode_steps: call rama_decode_begin first");
    rc = ensure_attn_part(c, cfg); if (rc) return rc;
    if (c->tune_ref_order && c->tune_chain) { rc = ensure_chain_copy(c, cfg, w, nullptr); if (rc) return rc; }
    if (c->samp_T != 0.0f) { rc = ensure_topp_scratch(c, cfg->vocab_size); if (rc) return rc; c->topp_dist_dirty = true; }      // (a replayed graph enqueues the pick without passing enqueue_sample)
    REQUIRE(c->host_pos + n_steps <= cfg->seq_len, RAMA_EINVAL, "decode_steps: would run past seq_len");
    const bool graphs = c->graph_mode && c->kp.kernel_id < 0;
    auto variant_at = [&](int pos) { return attn_variant(c, cfg, pos); };
    for (int i = 0; i < n_steps;) {
        // the attention variant depends on the position, which the host mirrors step by step
        const int v = apply_attn_variant(c, cfg, c->host_pos);
        int take = 1;
        if (graphs) {
            const int M = c->tune_graph_steps > 0 ? c->tune_graph_steps : (cfg->dim <= 1024 ? 4 : 1);
            if (M > 1 && n_steps - i >= M && variant_at(c->host_pos + M - 1) == v) take = M;   // the variant changes at most once, monotonically
            GraphCache& g = c->gc[v + (take > 1 ? 4 : 0)];
            if (!same_capture(g, cfg, w, s) || g.steps != take) {
                g.valid = false;
                rc = capture_graph(c, g.cg, [&] {
                    int re = 0;
                    for (int k = 0; k < take && !re; k++) re = enqueue_decode_step(c, cfg, w, s);
                    return re;
                });
                if (rc) return rc;
                g.cfg = *cfg; g.w = *w; g.s = *s; g.valid = true; g.copies_gen = rama_internal_copies_generation(); g.steps = take;
            }
            rc = replay_graph(c, g.cg); if (rc) return rc;
        } else {
            rc = enqueue_decode_step(c, cfg, w, s);
            if (rc) return rc;
        }
        c->host_pos += take;
        i += take;
    }
    c->ring_hi = std::min(c->out_cap, c->ring_hi + n_steps);
    return 0;
}

// Tokens the chained loop has produced so far, WITHOUT touching the stream: entries `from`.. of the host-visible ring the
// sampling launch writes next to its device list (generate_stream's channel, mod.rs:209-248: each token as it is produced).
// Returns at once; *n_ready may be 0.  Errors of the loop itself are reported by rama_decode_tokens at the end.
int rama_decode_stream_poll(rama_ctx* c, int from, int32_t* out_host, int max_tokens, int* n_ready) {
    RAMA_ENTER(c);
    REQUIRE(c && n_ready && from >= 0 && max_tokens >= 0 && (max_tokens == 0 || out_host), RAMA_EINVAL, "decode_stream_poll: bad argument");
    *n_ready = read_ring(c->ring, c->out_cap, from, out_host, max_tokens);
    return 0;
}

int rama_decode_tokens(rama_ctx* c, int32_t* out_host, int max_tokens, int* n_out) {
    RAMA_ENTER(c);
    REQUIRE(c && n_out, RAMA_EINVAL, "decode_tokens: NULL argument");
    Ctl h;
    HIPCHK(hipMemcpyAsync(&h, c->ctl, sizeof h, hipMemcpyDeviceToHost, c->stream));
    unsigned long long perr = 0;
    HIPCHK(hipMemcpyAsync(&perr, c->pbar + 1, sizeof perr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->handoff_dirty = false;
    if (perr != 0) {   // a bounded wait inside a launch gave up (attn_wo.hpp's counter, layer_fused.hpp's tagged vectors: 0x3000 / 0x3001): the results are invalid
        hipMemsetAsync(c->pbar, 0, 4 * sizeof(unsigned long long), c->stream);   // counter, error word, base: start over
        return fail(RAMA_EINVAL, perr >= kFusedErr ? "one-launch stage: a hand-off timed out" : "attention+Wo launch: hand-off timed out", __FILE__, __LINE__);
    }
    { const int rt = topp_dist_check(c); if (rt) return rt; }
    if (c->topp_err) {
        unsigned terr = 0;
        HIPCHK(hipMemcpy(&terr, c->topp_err, sizeof terr, hipMemcpyDeviceToHost));
        if (terr) {
            hipMemset(c->topp_err, 0, sizeof terr);
            return fail(RAMA_EINVAL, "top-p sampler: no probability above the cutoff (the reference underflows here, infer.rs:56-84)", __FILE__, __LINE__);
        }
    }
    int n = std::min(std::min(h.n_out, c->out_cap), max_tokens);
    if (n > 0 && out_host) {
        HIPCHK(hipMemcpyAsync(out_host, c->out, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *n_out = n;
    return 0;
}

int rama_generate_greedy(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                         const int32_t* prompt_host, int n_prompt, int steps, int32_t* out_host) {
    RAMA_ENTER(c);
    return rama_generate(c, cfg, w, s, prompt_host, n_prompt, steps, 0.0f, 0.9f, 0.0f, out_host);
}

// enqueue the whole generate() loop (mod.rs:169-206); the caller collects the tokens (all at the end, or as they appear)
// (*deferred != NULL: the decode steps are NOT enqueued, their count is returned there -- the streaming caller feeds them
// in pieces, see rama_generate_stream)
static int generate_enqueue(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                            const int32_t* prompt_host, int n_prompt, int steps, float temperature, float topp, float u,
                            int* deferred = nullptr) {
    REQUIRE(c && cfg, RAMA_EINVAL, "generate_greedy: NULL argument");
    { int rcs = rama_decode_sampler(c, temperature, topp, u); if (rcs) return rcs; }
    REQUIRE(steps >= 0 && steps <= cfg->seq_len, RAMA_EINVAL, "generate_greedy: steps > seq_len (the reference does not bound-check, SURVEY section 5)");
    REQUIRE(steps <= c->out_cap, RAMA_EINVAL, "generate_greedy: too many steps");
    REQUIRE(n_prompt >= 0 && (n_prompt == 0 || prompt_host), RAMA_EINVAL, "generate_greedy: bad prompt");
    n_prompt = std::min(n_prompt, c->forced_cap);
    int rc;
    if (c->tune_prefill && n_prompt >= 3 && steps > n_prompt) {
        // Positions 0..n_prompt carry known tokens (BOS, then the prompt; mod.rs:182-191) and their
        // `next` is forced, so they go through the layers together (rama_prefill); the logits of
        // position n_prompt give the first sampled token and the chained loop takes over.
        std::vector<int32_t> toks(n_prompt + 1);
        toks[0] = 1;
        for (int i = 0; i < n_prompt; i++) toks[i + 1] = prompt_host[i];
        for (int i = 0; i < n_prompt; i++) REQUIRE(prompt_host[i] >= 0 && prompt_host[i] < cfg->vocab_size, RAMA_EINVAL, "generate_greedy: prompt token outside the vocabulary");
        rc = ring_reset(c); if (rc) return rc;
        rc = rama_prefill(c, cfg, w, s, toks.data(), n_prompt + 1, 0);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(c->out, prompt_host, sizeof(int) * n_prompt, hipMemcpyHostToDevice, c->stream));   // forced `next`s
        for (int i = 0; i < n_prompt; i++) __atomic_store_n(c->ring + i, prompt_host[i] + 1, __ATOMIC_RELEASE);   // ... known at once
        c->ring_hi = n_prompt + 1;
        hipLaunchKernelGGL(set_ctl_kernel, dim3(1), dim3(1), 0, c->stream, c->ctl, toks[n_prompt], n_prompt, 0, n_prompt);
        LAUNCHCHK();
        ArgmaxParams ap{};
        ap.logits = s->logits; ap.n = cfg->vocab_size;
        ap.ctl = c->ctl; ap.forced = c->forced; ap.out = c->out; ap.out_cap = c->out_cap; ap.ring = c->ring_dev;
        ap.emb = w->token_embedding_table; ap.x = s->x; ap.dim = cfg->dim;
        if (c->samp_T != 0.0f) { rc = ensure_topp_scratch(c, cfg->vocab_size); if (rc) return rc; }
        rc = enqueue_sample(c, ap, c->samp_T, c->samp_topp, c->samp_u);               // out[n_prompt], cursor -> n_prompt + 1, next x
        if (rc) return rc;
        c->embedded_x = s->x;
        c->host_pos = n_prompt + 1;
        if (deferred) { *deferred = steps - n_prompt - 1; return 0; }
        rc = rama_decode_steps(c, cfg, w, s, steps - n_prompt - 1);
        if (rc) return rc;
    } else {
        rc = rama_decode_begin(c, /*BOS*/ 1, 0, prompt_host, n_prompt);
        if (rc) return rc;
        if (deferred) { *deferred = steps; return 0; }
        rc = rama_decode_steps(c, cfg, w, s, steps);
        if (rc) return rc;
    }
    return 0;
}

int rama_generate(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                  const int32_t* prompt_host, int n_prompt, int steps, float temperature, float topp, float u,
                  int32_t* out_host) {
    RAMA_ENTER(c);
    REQUIRE(out_host, RAMA_EINVAL, "generate_greedy: NULL argument");
    int rc = generate_enqueue(c, cfg, w, s, prompt_host, n_prompt, steps, temperature, topp, u);
    if (rc) return rc;
    int n = 0;
    return rama_decode_tokens(c, out_host, steps, &n);
}

// generate_stream (mod.rs:209-248): the same loop, every token handed to `on_token(user, index, token)` on the calling
// thread as soon as the device has produced it -- the loop itself runs on, chained on the device; the host only watches
// the ring.  out_host (may be NULL) receives the whole list at the end, as rama_generate does.
int rama_generate_stream(rama_ctx* c, const rama_config* cfg, const rama_weights* w, rama_run_state* s,
                         const int32_t* prompt_host, int n_prompt, int steps, float temperature, float topp, float u,
                         void (*on_token)(void* user, int index, int32_t token), void* user, int32_t* out_host) {
    RAMA_ENTER(c);
    REQUIRE(on_token, RAMA_EINVAL, "generate_stream: NULL callback");
    int todo = 0;
    int rc = generate_enqueue(c, cfg, w, s, prompt_host, n_prompt, steps, temperature, topp, u, &todo);
    if (rc) return rc;
    // The steps are fed to the stream a few at a time and never more than kAhead beyond the last token seen: a whole
    // generation enqueued at once fills the hardware queue (200 steps of llama2-7B are 32 000 packets), the enqueueing
    // thread then sits in hipGraphLaunch and the first token is looked at half a generation late.
    constexpr int kChunk = 8, kAhead = 24;
    int seen = 0, fed = steps - todo;                             // tokens handed over; tokens whose production is enqueued
    auto hand_over = [&]() -> int {
        int32_t buf[64];
        int n = 0;
        int r = rama_decode_stream_poll(c, seen, buf, std::min(64, steps - seen), &n); if (r) return r;
        for (int i = 0; i < n; i++) on_token(user, seen + i, buf[i]);
        seen += n;
        return 0;
    };
    while (seen < steps) {
        if (fed < steps && fed - seen < kAhead) {
            const int n = std::min(kChunk, steps - fed);
            rc = rama_decode_steps(c, cfg, w, s, n); if (rc) return rc;
            fed += n;
        }
        const int before = seen;
        rc = hand_over(); if (rc) return rc;
        if (seen == before && fed == steps) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); continue; }
            if (q != hipSuccess) return fail((int)q, "generate_stream: the stream failed while tokens were outstanding", __FILE__, __LINE__);
            rc = hand_over(); if (rc) return rc;                  // everything has run: what is there now is all there will be
            if (seen == before) break;
        }
    }
    std::vector<int32_t> tmp;
    if (!out_host) { tmp.resize(steps > 0 ? steps : 1); out_host = tmp.data(); }
    int n = 0;
    rc = rama_decode_tokens(c, out_host, steps, &n);                 // also reports what went wrong inside the loop, if anything
    if (rc) return rc;
    REQUIRE(seen == steps, RAMA_EINVAL, "generate_stream: the loop ended before every token had appeared");
    return 0;
}

// rama_set_tuning's keys, one row each: the member it stores, the values it takes -- a range, a short set, or a predicate with its wording --
// and whether setting it synchronises the stream and drops the captured graphs (kStoreOnly: the switches of the recording 1:1 ops and of the
// prompt path, which no captured launch depends on, only store).
struct TuneKey {
    const char* key;
    int rama_ctx::* member;
    bool drops;
    int lo, hi;                  // lo..hi (hi = INT_MAX: no upper end) ...
    int set[3]; int n_set;       // ... or, n_set > 0, one of set[0..n_set) ...
    bool (*ok)(int); const char* ok_text;      // ... or whatever ok() takes, worded ok_text
};
constexpr bool kDrop = true, kStoreOnly = false;
static constexpr TuneKey range(const char* key, int rama_ctx::* m, bool drops, int lo, int hi) { return {key, m, drops, lo, hi, {0, 0, 0}, 0, nullptr, nullptr}; }
static constexpr TuneKey one_of(const char* key, int rama_ctx::* m, bool drops, int a, int b) { return {key, m, drops, 0, 0, {a, b, 0}, 2, nullptr, nullptr}; }
static constexpr TuneKey one_of(const char* key, int rama_ctx::* m, bool drops, int a, int b, int c) { return {key, m, drops, 0, 0, {a, b, c}, 3, nullptr, nullptr}; }
static constexpr TuneKey pred(const char* key, int rama_ctx::* m, bool drops, bool (*ok)(int), const char* text) { return {key, m, drops, 0, 0, {0, 0, 0}, 0, ok, text}; }
static bool chain_resid_d_ok(int v) { return v == 0 || v == -1 || ((v / 100 == 1 || v / 100 == 2 || v / 100 == 4) && (v % 100 == 16 || v % 100 == 32)); }
static bool chain_d_ok(int v) { return v == 0 || (v >= 116 && v <= 432); }
static bool graph_steps_ok(int v) { return v == -1 || (v >= 1 && v <= 32); }

static constexpr TuneKey kTuneKeys[] = {
    range("ref_order", &rama_ctx::tune_ref_order, kDrop, 0, 3),      // (+ tune_tol, tune_bar: see rama_set_tuning)
    range("lane_reduce", &rama_ctx::tune_lane_reduce, kDrop, 0, 2),
    range("bar_pos", &rama_ctx::tune_bar_pos, kDrop, 0, INT_MAX),
    range("tol_mask", &rama_ctx::tune_tol_mask, kDrop, 0, 127),
    range("geom", &rama_ctx::tune_geom, kDrop, 0, 4),
    range("resid_r2", &rama_ctx::tune_resid_r2, kDrop, 0, 3),
    range("solo", &rama_ctx::tune_solo, kDrop, -1, 1),
    range("w13i", &rama_ctx::tune_w13i, kDrop, 0, 1),
    range("fused", &rama_ctx::tune_fused, kDrop, -1, 1),
    range("fused_solo", &rama_ctx::tune_fused_solo, kDrop, -1, 1),
    range("merge", &rama_ctx::tune_merge, kDrop, -1, 1),
    range("split_pos", &rama_ctx::tune_split_pos, kDrop, -1, INT_MAX),
    range("attn_nsplit", &rama_ctx::tune_attn_nsplit, kDrop, 0, 32),      // (+ attn_part goes: see rama_set_tuning)
    one_of("attn_waves", &rama_ctx::tune_attn_waves, kDrop, 4, 8, 16),
    range("attn_nt", &rama_ctx::tune_attn_nt, kDrop, 0, 1),
    one_of("attn_u", &rama_ctx::tune_attn_u, kDrop, 8, 16),
    range("combine_v", &rama_ctx::tune_combine_v, kDrop, 0, 1),
    range("small_attn", &rama_ctx::tune_small_attn, kDrop, -1, 1),
    one_of("small_attn_waves", &rama_ctx::tune_small_waves, kDrop, 4, 8),
    range("small_attn_pos", &rama_ctx::tune_small_pos, kDrop, 0, INT_MAX),
    pred("graph_steps", &rama_ctx::tune_graph_steps, kDrop, graph_steps_ok, "-1 or 1..32"),
    range("prefill", &rama_ctx::tune_prefill, kStoreOnly, 0, 1),
    one_of("prefill_tok", &rama_ctx::tune_prefill_tok, kDrop, 64, 128),
    range("prefill_attn", &rama_ctx::tune_prefill_attn, kStoreOnly, 0, 1),
    range("tiled", &rama_ctx::tune_tiled, kDrop, 0, 1),
    range("norm_in_gemm", &rama_ctx::tune_norm_in_gemm, kDrop, 0, 1),
    range("topp_sort", &rama_ctx::tune_topp_sort, kDrop, 0, 1),
    range("topp_pairs", &rama_ctx::tune_topp_pairs, kDrop, 0, 1),
    range("topp_dist", &rama_ctx::tune_topp_dist, kDrop, 0, 1),
    one_of("topp_block", &rama_ctx::tune_topp_block, kDrop, 512, 1024, 2048),
    range("topp_keep_sums", &rama_ctx::tune_topp_keep_sums, kDrop, 0, 1),
    range("chain", &rama_ctx::tune_chain, kDrop, 0, 1),
    pred("chain_d", &rama_ctx::tune_chain_d, kDrop, chain_d_ok, "0 or 100 W + D (116..432)"),
    pred("chain_resid_d", &rama_ctx::tune_chain_resid_d, kDrop, chain_resid_d_ok, "-1, 0 or 100 W + D, W in {1, 2, 4}, D in {16, 32}"),
    range("chain_lead_w", &rama_ctx::tune_chain_lead_w, kDrop, 0, 2),
    range("chain_norm", &rama_ctx::tune_chain_norm, kDrop, 0, 1),
    range("chain_lead", &rama_ctx::tune_chain_lead, kDrop, 0, 1),
    range("chain_split", &rama_ctx::tune_chain_split, kDrop, 0, 1),
    range("chain_views", &rama_ctx::tune_chain_views, kStoreOnly, 0, 1),
    range("spread_pos", &rama_ctx::tune_spread_pos, kDrop, 64, 1 << 20),
    range("attn_fv", &rama_ctx::tune_attn_fv, kDrop, 0, 1),
    range("prefill_chain", &rama_ctx::tune_prefill_chain, kStoreOnly, 0, 1),
    range("rope_batch", &rama_ctx::tune_rope_batch, kStoreOnly, 0, 1),
    range("matmul_batch", &rama_ctx::tune_matmul_batch, kStoreOnly, 0, 1),
    range("ew_batch", &rama_ctx::tune_ew_batch, kStoreOnly, 0, 1),
    range("norm_fold", &rama_ctx::tune_norm_fold, kStoreOnly, 0, 1),
    range("resid_fold", &rama_ctx::tune_resid_fold, kStoreOnly, 0, 1),
    range("qkv_fold", &rama_ctx::tune_qkv_fold, kStoreOnly, 0, 1),
};

static bool tune_value_ok(const TuneKey& k, int v) {
    if (k.ok) return k.ok(v);
    if (!k.n_set) return v >= k.lo && v <= k.hi;
    return std::find(k.set, k.set + k.n_set, v) != k.set + k.n_set;
}
static std::string tune_domain(const TuneKey& k) {
    if (k.ok) return k.ok_text;
    if (!k.n_set) return k.hi == INT_MAX ? ">= " + std::to_string(k.lo) : std::to_string(k.lo) + ".." + std::to_string(k.hi);
    std::string d = std::to_string(k.set[0]);
    for (int i = 1; i < k.n_set; i++) d += "|" + std::to_string(k.set[i]);
    return d;
}

// a refused value leaves the setting, the stream and the graphs alone
int rama_set_tuning(rama_ctx* c, const char* key, int value) {
    RAMA_ENTER(c);
    REQUIRE(c && key, RAMA_EINVAL, "set_tuning: NULL argument");
    const TuneKey* k = std::find_if(std::begin(kTuneKeys), std::end(kTuneKeys), [&](const TuneKey& e) { return !strcmp(key, e.key); });
    REQUIRE(k != std::end(kTuneKeys), RAMA_EINVAL, "set_tuning: unknown key");
    if (!tune_value_ok(*k, value)) return fail(RAMA_EINVAL, ("set_tuning: " + std::string(k->key) + " must be " + tune_domain(*k)).c_str(), __FILE__, __LINE__);
    if (k->drops) {
        HIPCHK(hipStreamSynchronize(c->stream));
        drop_graph(c);
    }
    c->*(k->member) = value;
    if (k->member == &rama_ctx::tune_ref_order) { c->tune_ref_order = value != 0; c->tune_tol = value == 2; c->tune_bar = value == 3; }
    if (k->member == &rama_ctx::tune_attn_nsplit && c->attn_part) { hipFree(c->attn_part); c->attn_part = nullptr; c->attn_part_floats = 0; }      // (sized by the slices per head)
    return 0;
}

int rama_set_graph_mode(rama_ctx* c, int enabled) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    c->graph_mode = enabled != 0;
    if (!enabled) { hipStreamSynchronize(c->stream); drop_graph(c); }
    return 0;
}

// ---------------------------------------------------------------- measurement

int rama_timer_start(rama_ctx* c) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    HIPCHK(hipEventRecord(c->t0, c->stream));
    return 0;
}
int rama_timer_stop(rama_ctx* c, float* ms) {
    RAMA_ENTER(c);
    REQUIRE(c && ms, RAMA_EINVAL, "timer_stop: NULL argument");
    HIPCHK(hipEventRecord(c->t1, c->stream));
    HIPCHK(hipEventSynchronize(c->t1));
    HIPCHK(hipEventElapsedTime(ms, c->t0, c->t1));
    return 0;
}

int rama_kprof_enable(rama_ctx* c, int kernel_id, int max_records) {
    RAMA_ENTER(c);
    REQUIRE(c && kernel_id >= 0 && kernel_id < RAMA_K_COUNT && max_records > 0, RAMA_EINVAL, "kprof_enable: bad argument");
    KProf& k = c->kp;
    while ((int)k.ev.size() < 2 * max_records) {
        hipEvent_t e; HIPCHK(hipEventCreate(&e)); k.ev.push_back(e);
    }
    k.kernel_id = kernel_id; k.max_records = max_records; k.used = 0;
    return 0;
}
int rama_kprof_read(rama_ctx* c, int* n_launches, double* total_ms) {
    RAMA_ENTER(c);
    REQUIRE(c && n_launches && total_ms, RAMA_EINVAL, "kprof_read: NULL argument");
    KProf& k = c->kp;
    HIPCHK(hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (int i = 0; i < k.used; i++) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, k.ev[2 * i], k.ev[2 * i + 1]));
        tot += ms;
    }
    *n_launches = k.used; *total_ms = tot;
    k.kernel_id = -1; k.used = 0;
    return 0;
}

// ---------------------------------------------------------------- state

int rama_state_create(rama_ctx* c, const rama_config* cfg, int n_local_layers, rama_run_state* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out, RAMA_EINVAL, "state_create: NULL argument");
    int rc = check_cfg(cfg); if (rc) return rc;
    REQUIRE(n_local_layers >= 0 && n_local_layers <= cfg->n_layers, RAMA_EINVAL, "state_create: bad layer count");
    // one blob, every buffer 256-byte aligned; sizes as ram.rs:7-23 (kv_dim == dim here)
    auto al = [](size_t n) { return (n + 63) & ~(size_t)63; };
    const size_t d = cfg->dim, h = cfg->hidden_dim;
    const size_t kv = (size_t)std::max(n_local_layers, 1) * cfg->seq_len * d;
    size_t sizes[12] = {d, d, d, h, h, d, d, d, (size_t)cfg->n_heads * cfg->seq_len, (size_t)cfg->vocab_size, kv, kv};
    size_t total = 0;
    for (size_t z : sizes) total += al(z);
    float* blob = nullptr;
    rc = rama_alloc_f32(c, total, &blob);
    if (rc) return rc;
    float** fields[12] = {&out->x, &out->xb, &out->xb2, &out->hb, &out->hb2, &out->q, &out->k, &out->v, &out->att, &out->logits, &out->key_cache, &out->value_cache};
    size_t off = 0;
    for (int i = 0; i < 12; i++) { *fields[i] = blob + off; off += al(sizes[i]); }
    return 0;
}

int rama_state_free(rama_ctx* c, rama_run_state* s) {
    RAMA_ENTER(c);
    REQUIRE(c && s, RAMA_EINVAL, "state_free: NULL argument");
    drop_q8_graphs(c, s);          // the Q8 steps captured over this state (the fp32 graphs: rama_set_graph_mode(0) first, as documented)
    serve_state_gone(c, s);        // ... and the fp32 serving chain ends when a slot still on the device's hands uses it
    int rc = rama_free(c, s->x);   // x is the blob base
    memset(s, 0, sizeof *s);
    return rc;
}
