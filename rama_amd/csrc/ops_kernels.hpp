// ops_kernels.hpp -- the kernels of kernels.hpp that are no templates and that rama_api.hip alone launches: the 1:1 ops, the synthetic fill.
// A kernel that is no template is emitted by every translation unit that sees its definition, so these live
// apart from the types, device functions and template kernels of kernels.hpp, which the other translation units see too.
#pragma once
#include "kernels.hpp"

namespace rama {

// generic o_cols > 1 product of the trait signature (never used by forward): one thread per output
__global__ void matmul_generic(float* o, const float* a, const float* b, int width, int o_rows, int o_cols) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= o_rows * o_cols) return;
    int r = idx / o_cols, c = idx % o_cols;
    float acc = 0.0f;
    for (int k = 0; k < width; k++) acc = fmaf(a[(size_t)r * width + k], b[(size_t)k * o_cols + c], acc);
    o[idx] = acc;
}

// unaligned-view fallback of the o_cols == 1 product (16-byte alignment not given): one wave per row
__global__ __launch_bounds__(kWG) void matvec_unaligned(float* o, const float* a, const float* x, int width, int rows) {
    int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    int lane = threadIdx.x & 63;
    float acc = 0.0f;
    for (int k = lane; k < width; k += 64) acc = fmaf(a[(size_t)row * width + k], x[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) o[row] = acc;
}

// split-T combine: xb[h] = sum_s e^(m_s - M) acc_s / sum_s e^(m_s - M) l_s,  M = max_s m_s
// (algebraically the softmax over all timesteps; an empty slice has l = 0 and drops out)
// the plain loop (round 1), kept for A/B (rama_set_tuning "combine_v" = 0)
__global__ void attention_combine_loop_kernel(const float* part, float* xb, int head_size, int nsplit) {
    const int h = blockIdx.x, i = threadIdx.x;
    const size_t ps = (size_t)(head_size + 4);
    const float* ph = part + (size_t)h * nsplit * ps;
    float M = -INFINITY;
    for (int s = 0; s < nsplit; s++) if (ph[s * ps + 1] > 0.0f) M = fmaxf(M, ph[s * ps]);
    float L = 0.0f, o = 0.0f;
    for (int s = 0; s < nsplit; s++) {
        const float l = ph[s * ps + 1];
        if (l > 0.0f) {
            const float sc = expf(ph[s * ps] - M);
            L += sc * l;
            if (i < head_size) o += sc * ph[s * ps + 4 + i];
        }
    }
    if (i < head_size) xb[(size_t)h * head_size + i] = o / L;
}

// cursor from a token id that lives in device memory (pipeline stages); an id outside the
// vocabulary is clamped so a corrupted hand-off cannot turn into a wild embedding read
__global__ void set_ctl_dev_kernel(Ctl* ctl, const int* token_dev, int pos, int vocab) {
    int t = token_dev ? *token_dev : 0;
    t = t < 0 ? 0 : (t >= vocab ? vocab - 1 : t);
    ctl->token = t; ctl->pos = pos; ctl->n_forced = 0; ctl->n_out = 0;
}

__global__ void array_add_kernel(float* t, const float* s, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) t[i] += s[i];
}

__global__ void array_mult_kernel(float* t, const float* s, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) t[i] *= s[i];
}

__global__ void sinu_kernel(float* o, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float a = o[i];
        o[i] = a * (1.0f / (1.0f + expf(-a)));
    }
}

// two Device::copy_from_slice calls as one launch (infer.rs:32-33: the key row and the value row of the cache)
__global__ void copy2_kernel(float* t1, const float* s1, size_t n1, float* t2, const float* s2, size_t n2) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n1 + n2; i += (size_t)gridDim.x * blockDim.x) {
        if (i < n1) t1[i] = s1[i]; else t2[i - n1] = s2[i - n1];
    }
}

// Device::sinu followed by Device::array_mult on the same vector (infer.rs:44-45) as one launch, each product rounded as in the two
__global__ void sinu_mult_kernel(float* o, const float* s, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float a = o[i];
        a = a * (1.0f / (1.0f + expf(-a)));
        o[i] = a * s[i];
    }
}

// cpu.rs:99-117, one workgroup
__global__ __launch_bounds__(1024) void rmsnorm_kernel(float* o, const float* x, const float* w, int n) {
    __shared__ float red[16];
    float ss = 0.0f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) ss = fmaf(x[i], x[i], ss);
    ss = block_sum(ss, red);
    const float v = rms_scale(ss, n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) o[i] = w[i] * (v * x[i]);
}

// cpu.rs:74-97, one head
__global__ void apply_position_kernel(float* q, float* k, const float* pr, const float* pi, int head_size) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= head_size / 2) return;
    float c = pr[i], s = pi[i];
    float q0 = q[2 * i], q1 = q[2 * i + 1];
    q[2 * i] = q0 * c - q1 * s; q[2 * i + 1] = q0 * s + q1 * c;
    float k0 = k[2 * i], k1 = k[2 * i + 1];
    k[2 * i] = k0 * c - k1 * s; k[2 * i + 1] = k0 * s + k1 * c;
}

// ... for a run of consecutive heads (dim = heads x head_size floats of q and of k; the same table rows for every head: infer.rs:25-29's loop as one launch)
__global__ void apply_position_heads_kernel(float* q, float* k, const float* pr, const float* pi, int head_size, int dim) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dim / 2) return;
    const int i = j % (head_size / 2);
    float c = pr[i], s = pi[i];
    float q0 = q[2 * j], q1 = q[2 * j + 1];
    q[2 * j] = q0 * c - q1 * s; q[2 * j + 1] = q0 * s + q1 * c;
    float k0 = k[2 * j], k1 = k[2 * j + 1];
    k[2 * j] = k0 * c - k1 * s; k[2 * j + 1] = k0 * s + k1 * c;
}

// cpu.rs:119-125, one workgroup
__global__ __launch_bounds__(1024) void softmax_kernel(float* x, int n) {
    __shared__ float red[16];
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, x[i]);
    mx = block_max(mx, red);
    float sum = 0.0f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) { float e = expf(x[i] - mx); x[i] = e; sum += e; }
    sum = block_sum(sum, red);
    for (int i = threadIdx.x; i < n; i += blockDim.x) x[i] /= sum;
}

// bit-exact twin of oracle_fill_synth (integer hash, Irwin-Hall(4), one multiply, one add)
__global__ void fill_synth_kernel(float* dst, size_t n, uint64_t base, float scale, float bias) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t z = (uint64_t)i + base;
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
        z ^= z >> 27; z *= 0x94D049BB133111EBULL;
        z ^= z >> 31;
        int sum = (int)(z & 0xFFFF) + (int)((z >> 16) & 0xFFFF) + (int)((z >> 32) & 0xFFFF) + (int)(z >> 48);
        float prod = (float)(sum - 131070) * scale;
        asm volatile("" : "+v"(prod));   // opaque: bias + prod must round twice like the CPU generator, never one FMA
        dst[i] = bias + prod;
    }
}

}  // namespace rama
