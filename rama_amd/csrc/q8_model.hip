// q8_model.hip -- Q8_0 weights in HBM: the llama2.c version-2 checkpoint loader (export.py version2_export's layout) and the
// synthetic Q8 model (rama_model_synth's fp32 weights quantized by export.py quantize_q80's rule).
#include "../../include/rama_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

extern "C" int rama_fill_synth(rama_ctx*, float*, size_t, uint64_t, uint64_t, uint64_t, float, float);
extern "C" void* rama_internal_stream(rama_ctx* c);
extern "C" int rama_internal_device(rama_ctx* c);
extern "C" void rama_internal_rope_tables(const rama_config* cfg, std::vector<float>* re, std::vector<float>* im);   // model.hip
extern "C" void rama_internal_drop_q8_graphs(rama_ctx* ctx, const rama_q8_weights* freed);                                                      // rama_api.hip

struct rama_q8_model {
    rama_config cfg{};
    rama_q8_weights w{};
    float* blob = nullptr;      // one allocation: fp32 norms, RoPE tables and the dequantized token table, then int8 values and scales
    size_t streamed = 0;        // bytes a decode step reads of it (rama_q8_model_bytes)
};

namespace {

int bad(int code, const char* msg) { fprintf(stderr, "rama_q8_model: %s\n", msg); return code; }
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// export.py quantize_q80: scale = max|w| / 127, q = torch.round(w / scale) (halves to even); scale 0 gives q = 0
__global__ void q8_quantize_weights_kernel(const float* __restrict__ w, size_t ngroups, int gs, int8_t* __restrict__ q, float* __restrict__ s) {
#pragma clang fp contract(off)
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * blockDim.x) {
        const float* wg = w + g * gs;
        float m = 0.0f;
        for (int i = 0; i < gs; i++) m = fmaxf(m, fabsf(wg[i]));
        const float scale = m / 127.0f;
        for (int i = 0; i < gs; i++) {
            float r = scale == 0.0f ? 0.0f : rintf(wg[i] / scale);
            r = fminf(fmaxf(r, -127.0f), 127.0f);
            q[g * gs + i] = (int8_t)(int)r;
        }
        s[g] = scale;
    }
}

// fp32 copy of a quantized table: out[i] = q[i] * s[i / gs] (runq.c's dequantized token embedding)
__global__ void q8_dequantize_kernel(float* __restrict__ out, const int8_t* __restrict__ q, const float* __restrict__ s, size_t n, int gs) {
#pragma clang fp contract(off)
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = (float)q[i] * s[i / gs];
}

struct QSpec { const char* name; size_t n; int tag; double std; bool layered; };

// the quantized tensors in file order (export.py:196-208; a layered one is written layer by layer); wcls only when not shared
std::vector<QSpec> q8_layout(const rama_config& c) {
    const size_t L = c.n_layers, d = c.dim, h = c.hidden_dim, V = c.vocab_size;
    const double res = 0.02 / std::sqrt(2.0 * (double)L);      // model.py:232-236, as rama_model_synth
    std::vector<QSpec> t = {
        {"tok", V * d, 1, 0.02, false}, {"wq", L * d * d, 3, 0.02, true}, {"wk", L * d * d, 4, 0.02, true}, {"wv", L * d * d, 5, 0.02, true},
        {"wo", L * d * d, 6, res, true}, {"w1", L * h * d, 8, 0.02, true}, {"w2", L * d * h, 9, 0.02, true}, {"w3", L * h * d, 10, res, true},
    };
    if (!c.shared_weight) t.push_back({"wcls", V * d, 12, 0.02, false});
    return t;
}

void set_q(rama_q8_weights& w, const char* name, const int8_t* q, const float* s) {
#define F(n) if (!strcmp(name, #n)) { w.n = q; w.n##_s = s; return; }
    F(tok) F(wq) F(wk) F(wv) F(wo) F(w1) F(w2) F(w3) F(wcls)
#undef F
}

int check_q8_cfg(const rama_config& c, int gs) {
    if (c.dim <= 0 || c.hidden_dim <= 0 || c.n_layers <= 0 || c.n_heads <= 0 || c.vocab_size <= 0 || c.seq_len <= 0 || c.dim % c.n_heads)
        return bad(RAMA_EIO, "implausible header");
    if (c.n_kv_heads != c.n_heads) return bad(RAMA_EUNSUP, "n_kv_heads != n_heads (the reference indexes the cache with stride dim)");
    if (gs <= 0 || c.dim % gs || c.hidden_dim % gs) return bad(RAMA_EUNSUP, "group_size does not divide dim and hidden_dim");
    return 0;
}

// lays out the model's allocation: fp32 part (norms, RoPE, dequantized table), then each quantized tensor's values and scales
int q8_alloc(rama_ctx* ctx, const rama_config& c, int gs, rama_q8_model** out, std::vector<std::pair<int8_t*, float*>>* qt) {
    const size_t L = c.n_layers, d = c.dim, hs = d / c.n_heads, S = c.seq_len, V = c.vocab_size;
    const size_t fp_floats[] = {L * d, L * d, d, S * (hs / 2), S * (hs / 2), V * d};
    size_t bytes = 0;
    for (size_t n : fp_floats) bytes += up256(n * 4);
    auto lay = q8_layout(c);
    for (auto& t : lay) bytes += up256(t.n) + up256(t.n / gs * 4);
    rama_q8_model* m = new rama_q8_model();
    m->cfg = c;
    int rc = rama_alloc_f32(ctx, (bytes + 3) / 4, &m->blob);
    if (rc) { delete m; return rc; }
    char* p = (char*)m->blob;
    const float** fp[] = {&m->w.rms_att_weight, &m->w.rms_ffn_weight, &m->w.rms_final_weight, &m->w.freq_cis_real, &m->w.freq_cis_imag,
                          &m->w.token_embedding_table};
    for (int i = 0; i < 6; i++) { *fp[i] = (const float*)p; p += up256(fp_floats[i] * 4); }
    m->w.group_size = gs;
    m->streamed = (2 * L * d + d) * 4;
    qt->clear();
    for (auto& t : lay) {
        int8_t* q = (int8_t*)p; p += up256(t.n);
        float* s = (float*)p; p += up256(t.n / gs * 4);
        set_q(m->w, t.name, q, s);
        qt->push_back({q, s});
        if (strcmp(t.name, "tok") || c.shared_weight) m->streamed += t.n + t.n / gs * 4;      // the token table is streamed only as the classifier
    }
    if (c.shared_weight) { m->w.wcls = m->w.tok; m->w.wcls_s = m->w.tok_s; }
    *out = m;
    return 0;
}

// the fp32 token table and the RoPE tables (model.py:41-47, as rama_model_synth computes them without given tables)
int q8_finish(rama_ctx* ctx, rama_q8_model* m) {
    const rama_config& c = m->cfg;
    std::vector<float> re, im;
    rama_internal_rope_tables(&c, &re, &im);
    int rc = rama_copy_h2d_f32(ctx, (float*)m->w.freq_cis_real, re.data(), re.size());
    if (!rc) rc = rama_copy_h2d_f32(ctx, (float*)m->w.freq_cis_imag, im.data(), im.size());
    if (rc) return rc;
    hipStream_t st = (hipStream_t)rama_internal_stream(ctx);
    hipLaunchKernelGGL(q8_dequantize_kernel, dim3(4096), dim3(256), 0, st, (float*)m->w.token_embedding_table, m->w.tok, m->w.tok_s,
                       (size_t)c.vocab_size * c.dim, m->w.group_size);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bad(RAMA_EIO, "dequantizing the token table failed");
    return 0;
}

}  // namespace

extern "C" int rama_q8_model_load(rama_ctx* ctx, const char* path, rama_q8_model** out) {
    if (!ctx || !path || !out) return bad(RAMA_EINVAL, "rama_q8_model_load: NULL argument");
    int fd = open(path, O_RDONLY);
    if (fd < 0) return bad(RAMA_EIO, "cannot open checkpoint");
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size < 8) { close(fd); return bad(RAMA_EIO, "checkpoint too small"); }
    void* map = mmap(nullptr, sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (map == MAP_FAILED) return bad(RAMA_EIO, "mmap failed");
    const char* f = (const char*)map;
    int32_t h[9] = {}, gs = 0;
    memcpy(h, f, 8);
    auto done = [&](int code) { munmap(map, sb.st_size); return code; };
    if ((uint32_t)h[0] != 0x616b3432u) return done(bad(RAMA_EUNSUP, "not an ak42 file (a v0 checkpoint goes through rama_model_load)"));
    if (h[1] != 2) return done(bad(RAMA_EUNSUP, "ak42 file of a version other than 2 (Q8_0)"));
    if (sb.st_size < 256) return done(bad(RAMA_EIO, "checkpoint shorter than the 256-byte version-2 header"));
    memcpy(h, f, sizeof h);
    memcpy(&gs, f + 37, 4);      // export.py:229-230: the shared byte at 36, the group size right behind it
    rama_config c{};
    c.dim = h[2]; c.hidden_dim = h[3]; c.n_layers = h[4]; c.n_heads = h[5]; c.n_kv_heads = h[6]; c.vocab_size = h[7]; c.seq_len = h[8];
    c.shared_weight = f[36] != 0;
    int rc = check_q8_cfg(c, gs);
    if (rc) return done(rc);
    const size_t L = c.n_layers, d = c.dim;
    const size_t norm_floats = 2 * L * d + d;
    size_t total = 256 + norm_floats * 4;
    for (auto& t : q8_layout(c)) total += t.n + t.n / gs * 4;
    if ((size_t)sb.st_size != total) return done(bad(RAMA_EIO, "checkpoint size does not match its header (export.py version2_export layout)"));
    rama_q8_model* m = nullptr;
    std::vector<std::pair<int8_t*, float*>> qt;
    rc = q8_alloc(ctx, c, gs, &m, &qt);
    if (rc) return done(rc);
    size_t off = 256;
    std::vector<float> tmp(norm_floats);
    memcpy(tmp.data(), f + off, norm_floats * 4);
    off += norm_floats * 4;
    rc = rama_copy_h2d_f32(ctx, (float*)m->w.rms_att_weight, tmp.data(), L * d);
    if (!rc) rc = rama_copy_h2d_f32(ctx, (float*)m->w.rms_ffn_weight, tmp.data() + L * d, L * d);
    if (!rc) rc = rama_copy_h2d_f32(ctx, (float*)m->w.rms_final_weight, tmp.data() + 2 * L * d, d);
    if (!rc) rc = rama_sync(ctx);
    if (!rc && hipSetDevice(rama_internal_device(ctx)) != hipSuccess) rc = bad(RAMA_EIO, "hipSetDevice failed");
    auto lay = q8_layout(c);
    for (size_t i = 0; i < lay.size() && !rc; i++) {
        // export.py quantizes every layer's matrix on its own: values then scales per layer; HBM keeps the layers stacked
        const size_t parts = lay[i].layered ? L : 1, n = lay[i].n / parts, ns = n / gs;
        for (size_t l = 0; l < parts && !rc; l++) {
            if (hipMemcpy(qt[i].first + l * n, f + off, n, hipMemcpyHostToDevice) != hipSuccess) rc = bad(RAMA_EIO, "copy to the device failed");
            off += n;
            if (!rc && hipMemcpy(qt[i].second + l * ns, f + off, ns * 4, hipMemcpyHostToDevice) != hipSuccess) rc = bad(RAMA_EIO, "copy to the device failed");
            off += ns * 4;
        }
    }
    munmap(map, sb.st_size);
    if (!rc) rc = q8_finish(ctx, m);
    if (rc) { rama_q8_model_free(ctx, m); return rc; }
    *out = m;
    return 0;
}

extern "C" int rama_q8_model_synth(rama_ctx* ctx, const rama_config* cfg, int group_size, uint64_t seed, rama_q8_model** out) {
    if (!ctx || !cfg || !out) return bad(RAMA_EINVAL, "rama_q8_model_synth: NULL argument");
    const rama_config& c = *cfg;
    int rc = check_q8_cfg(c, group_size);
    if (rc) return rc == RAMA_EIO ? RAMA_EINVAL : rc;
    rama_q8_model* m = nullptr;
    std::vector<std::pair<int8_t*, float*>> qt;
    rc = q8_alloc(ctx, c, group_size, &m, &qt);
    if (rc) return rc;
    const double ih4_std = std::sqrt(4.0 * (65536.0 * 65536.0 - 1.0) / 12.0);
    const size_t L = c.n_layers, d = c.dim;
    // the norms: rama_model_synth's tags 2, 7, 11 (gains 1 + noise)
    const float nscale = (float)(0.05 / ih4_std);
    rc = rama_fill_synth(ctx, (float*)m->w.rms_att_weight, L * d, seed, 2, 0, nscale, 1.f);
    if (!rc) rc = rama_fill_synth(ctx, (float*)m->w.rms_ffn_weight, L * d, seed, 7, 0, nscale, 1.f);
    if (!rc) rc = rama_fill_synth(ctx, (float*)m->w.rms_final_weight, d, seed, 11, 0, nscale, 1.f);
    // the matrices through a bounded scratch: pieces of whole groups, each filled at its offset in the tensor and quantized
    const size_t chunk = ((size_t)1 << 24) / group_size * group_size;
    float* scratch = nullptr;
    if (!rc) rc = rama_alloc_f32(ctx, chunk, &scratch);
    auto lay = q8_layout(c);
    hipStream_t st = (hipStream_t)rama_internal_stream(ctx);
    for (size_t i = 0; i < lay.size() && !rc; i++) {
        for (size_t off = 0; off < lay[i].n && !rc; off += chunk) {
            const size_t n = std::min(chunk, lay[i].n - off);
            rc = rama_fill_synth(ctx, scratch, n, seed, (uint64_t)lay[i].tag, off, (float)(lay[i].std / ih4_std), 0.f);
            if (rc) break;
            st = (hipStream_t)rama_internal_stream(ctx);
            hipLaunchKernelGGL(q8_quantize_weights_kernel, dim3(2048), dim3(256), 0, st, (const float*)scratch, n / group_size, group_size,
                               qt[i].first + off, qt[i].second + off / group_size);
            if (hipGetLastError() != hipSuccess) rc = bad(RAMA_EIO, "quantize launch failed");
        }
    }
    if (!rc) rc = rama_sync(ctx);
    if (scratch) rama_free(ctx, scratch);
    if (!rc) rc = q8_finish(ctx, m);
    if (rc) { rama_q8_model_free(ctx, m); return rc; }
    *out = m;
    return 0;
}

// A resident fp32 weight set quantized where it lies: rama_weights keeps every layered tensor stacked over the layers, and group_size divides a
// layer's matrix (dim and hidden_dim are multiples of it), so no group spans two layers and one launch over the stacked tensor quantizes every layer's
// matrix on its own, as export.py does.  The quantizer is q8_quantize_weights_kernel as it stands: its group index is a size_t and it walks
// a grid of 2048 x 256 threads in strides, so a tensor of 2^31 groups takes 4096 rounds of it.
extern "C" int rama_q8_model_from_f32(rama_ctx* ctx, const rama_config* cfg, const rama_weights* w, int group_size, rama_q8_model** out) {
    if (!ctx || !cfg || !w || !out) return bad(RAMA_EINVAL, "rama_q8_model_from_f32: NULL argument");
    const rama_config& c = *cfg;
    if (c.dim <= 0 || c.hidden_dim <= 0 || c.n_layers <= 0 || c.n_heads <= 0 || c.vocab_size <= 0 || c.seq_len <= 0 || c.dim % c.n_heads)
        return bad(RAMA_EINVAL, "rama_q8_model_from_f32: implausible config");
    if (!w->token_embedding_table || !w->rms_att_weight || !w->rms_ffn_weight || !w->wq || !w->wk || !w->wv || !w->wo || !w->w1 || !w->w2 || !w->w3 ||
        !w->rms_final_weight || !w->wcls)
        return bad(RAMA_EINVAL, "rama_q8_model_from_f32: incomplete weights (a pipeline stage's, or tensors still missing)");
    if (c.n_kv_heads != c.n_heads) return bad(RAMA_EUNSUP, "n_kv_heads != n_heads (the reference indexes the cache with stride dim)");
    if (group_size <= 0) return bad(RAMA_EINVAL, "rama_q8_model_from_f32: group_size <= 0");
    if (c.dim % group_size || c.hidden_dim % group_size) return bad(RAMA_EINVAL, "rama_q8_model_from_f32: group_size does not divide dim and hidden_dim");
    rama_config qc = c;
    const bool one_tensor = w->wcls == w->token_embedding_table;
    if (c.shared_weight && !one_tensor) return bad(RAMA_EINVAL, "rama_q8_model_from_f32: shared_weight is set but wcls is a tensor of its own");
    qc.shared_weight = one_tensor;      // (one tensor behind both names is shared whatever the config says)
    rama_q8_model* m = nullptr;
    std::vector<std::pair<int8_t*, float*>> qt;
    int rc = q8_alloc(ctx, qc, group_size, &m, &qt);
    if (rc) return rc;
    const size_t L = qc.n_layers, d = qc.dim;
    rc = rama_sync(ctx);       // the source's tensors may still be being written by the context's stream or a copy
    if (!rc && hipSetDevice(rama_internal_device(ctx)) != hipSuccess) rc = bad(RAMA_EIO, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)rama_internal_stream(ctx);
    const struct { const float* dst; const float* src; size_t n; } norms[] = {
        {m->w.rms_att_weight, w->rms_att_weight, L * d}, {m->w.rms_ffn_weight, w->rms_ffn_weight, L * d}, {m->w.rms_final_weight, w->rms_final_weight, d}};
    for (auto& n : norms)
        if (!rc && hipMemcpyAsync((float*)n.dst, n.src, n.n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = bad(RAMA_EIO, "copying the norms failed");
    const float* src[] = {w->token_embedding_table, w->wq, w->wk, w->wv, w->wo, w->w1, w->w2, w->w3, w->wcls};      // q8_layout's order
    auto lay = q8_layout(qc);
    for (size_t i = 0; i < lay.size() && !rc; i++) {
        hipLaunchKernelGGL(q8_quantize_weights_kernel, dim3(2048), dim3(256), 0, st, src[i], lay[i].n / (size_t)group_size, group_size, qt[i].first,
                           qt[i].second);
        if (hipGetLastError() != hipSuccess) rc = bad(RAMA_EIO, "quantize launch failed");
    }
    if (!rc) rc = rama_sync(ctx);
    if (!rc) rc = q8_finish(ctx, m);
    if (rc) { rama_q8_model_free(ctx, m); return rc; }
    *out = m;
    return 0;
}

extern "C" int rama_q8_model_config(const rama_q8_model* m, rama_config* cfg) {
    if (!m || !cfg) return RAMA_EINVAL;
    *cfg = m->cfg;
    return 0;
}
extern "C" int rama_q8_model_weights(const rama_q8_model* m, rama_q8_weights* w) {
    if (!m || !w) return RAMA_EINVAL;
    *w = m->w;
    return 0;
}
extern "C" size_t rama_q8_model_bytes(const rama_q8_model* m) { return m ? m->streamed : 0; }
extern "C" int rama_q8_model_free(rama_ctx* ctx, rama_q8_model* m) {
    if (!m) return 0;
    if (ctx) { rama_sync(ctx); rama_internal_drop_q8_graphs(ctx, &m->w); }      // captured Q8 steps hold the model's addresses (the fp32 graphs stay); a chained batch over it ends
    const int rc = m->blob ? rama_free(ctx, m->blob) : 0;
    delete m;
    return rc;
}
