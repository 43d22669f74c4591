// ref_kernels.hpp -- the kernels of ref_order.hpp (none is a template) but rope_ref_cursor_kernel: rama_api.hip alone launches them.
// A kernel that is no template is emitted by every translation unit that sees its definition, so these live
// apart from the types, device functions and template kernels of ref_order.hpp, which the Q8 translation units see too.
#pragma once
#include "ref_order.hpp"

namespace rama {

__global__ void expf_glibc_kernel(float* o, const float* x, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) o[i] = expf_glibc(x[i]);
}

// ---------------------------------------------------------------- cpu.rs:127-153 matmul, o_cols == 1 (the order: ref_order.hpp RefMatParams)
__global__ __launch_bounds__(64) void matvec_ref_kernel(RefMatParams p) {
    RAMA_NO_CONTRACT
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= p.rows) return;
    const int m = blockIdx.y;
    const float* W = (m == 0 ? p.w[0] : (m == 1 ? p.w[1] : p.w[2])) + (size_t)r * p.K;
    float* o = m == 0 ? p.o[0] : (m == 1 ? p.o[1] : p.o[2]);
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;
    const bool vec = (((uintptr_t)W | (uintptr_t)p.x) & 15) == 0;
    if (vec) {
        const f4* w4 = reinterpret_cast<const f4*>(W);
        const f4* x4 = reinterpret_cast<const f4*>(p.x);
        const int n4 = p.K >> 2;
        int i = 0;
        for (; i + 8 <= n4; i += 8) {
            f4 a[8];
#pragma unroll
            for (int u = 0; u < 8; u++) a[u] = w4[i + u];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const f4 b = x4[i + u];
                v0 = v0 + a[u].x * b.x; v1 = v1 + a[u].y * b.y; v2 = v2 + a[u].z * b.z; v3 = v3 + a[u].w * b.w;
            }
        }
        for (; i < n4; i++) {
            const f4 a = w4[i], b = x4[i];
            v0 = v0 + a.x * b.x; v1 = v1 + a.y * b.y; v2 = v2 + a.z * b.z; v3 = v3 + a.w * b.w;
        }
    } else {
        for (int k = 0; k < p.K; k += 4) {
            v0 = v0 + W[k] * p.x[k]; v1 = v1 + W[k + 1] * p.x[k + 1];
            v2 = v2 + W[k + 2] * p.x[k + 2]; v3 = v3 + W[k + 3] * p.x[k + 3];
        }
    }
    o[r] = p.lane_reduce == LANES_STRIDED ? (v0 + v2) + (v1 + v3) : (p.lane_reduce == LANES_SEQUENTIAL ? ((v0 + v1) + v2) + v3 : (v0 + v1) + (v2 + v3));
}

// the trait's o_cols > 1 product (cpu.rs:137-151 as written: output idx = r * o_cols + c, b strided by o_cols; forward() never calls it): one thread per
// output, the same four chains and the same final order
__global__ __launch_bounds__(256) void matmul_cols_ref_kernel(float* o, const float* a, const float* b, int width, int o_rows, int o_cols, int lane_reduce) {
    RAMA_NO_CONTRACT
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)o_rows * (size_t)o_cols) return;
    const size_t r = idx / (size_t)o_cols, cc = idx % (size_t)o_cols;
    const float* ar = a + r * (size_t)width;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;
    for (int k = 0; k < width; k += 4) {
        v0 = v0 + ar[k] * b[(size_t)k * o_cols + cc];
        v1 = v1 + ar[k + 1] * b[(size_t)(k + 1) * o_cols + cc];
        v2 = v2 + ar[k + 2] * b[(size_t)(k + 2) * o_cols + cc];
        v3 = v3 + ar[k + 3] * b[(size_t)(k + 3) * o_cols + cc];
    }
    o[idx] = lane_reduce == LANES_STRIDED ? (v0 + v2) + (v1 + v3) : (lane_reduce == LANES_SEQUENTIAL ? ((v0 + v1) + v2) + v3 : (v0 + v1) + (v2 + v3));
}

// ---------------------------------------------------------------- cpu.rs:99-117 rmsnorm
__global__ __launch_bounds__(1024) void rmsnorm_ref_kernel(float* o, const float* x, const float* w, int n) {
    RAMA_NO_CONTRACT
    extern __shared__ __attribute__((aligned(16))) float s_x[];
    __shared__ float s_vv;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s_x[i] = x[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        float ss = 0.0f;
        for (int i = 0; i < n; i++) ss = ss + s_x[i] * s_x[i];
        s_vv = 1.0f / sqrtf(ss / (float)n + 1e-5f);
    }
    __syncthreads();
    const float v = s_vv;
    for (int i = threadIdx.x; i < n; i += blockDim.x) o[i] = w[i] * (v * s_x[i]);
}

// ---------------------------------------------------------------- cpu.rs:74-97 apply_position, all heads
// + the two cache appends of infer.rs:31-33 when kc / vc are given
__global__ void rope_ref_kernel(float* q, float* k, const float* v, const float* pr, const float* pi, int dim, int head_size,
                                float* kc_row, float* vc_row) {
    RAMA_NO_CONTRACT
    const int j = blockIdx.x * blockDim.x + threadIdx.x;      // pair index over the whole vector
    if (j >= dim / 2) return;
    const int i = j % (head_size / 2);
    const float fcr = pr[i], fci = pi[i];
    const float q0 = q[2 * j], q1 = q[2 * j + 1];
    const float a0 = q0 * fcr - q1 * fci, a1 = q0 * fci + q1 * fcr;
    q[2 * j] = a0; q[2 * j + 1] = a1;
    const float k0 = k[2 * j], k1 = k[2 * j + 1];
    const float b0 = k0 * fcr - k1 * fci, b1 = k0 * fci + k1 * fcr;
    k[2 * j] = b0; k[2 * j + 1] = b1;
    if (kc_row) { kc_row[2 * j] = b0; kc_row[2 * j + 1] = b1; }
    if (vc_row) { vc_row[2 * j] = v[2 * j]; vc_row[2 * j + 1] = v[2 * j + 1]; }
}

// ---------------------------------------------------------------- cpu.rs:23-52 multi_head_attention (ref_order.hpp RefAttnParams)
__global__ __launch_bounds__(1024) void attention_ref_kernel(RefAttnParams p) {
    RAMA_NO_CONTRACT
    extern __shared__ __attribute__((aligned(16))) float s_att[];
    __shared__ float red[16];
    __shared__ float s_sum;
    const int h = blockIdx.x, tid = threadIdx.x;
    const int pos = p.ctl ? p.ctl->pos : p.pos_val;
    const int hs = p.head_size;
    const float* q = p.q + (size_t)h * hs;
    const float scale_div = sqrtf((float)hs);
    for (int t = tid; t <= pos; t += blockDim.x) {
        const float* k = p.kc + (size_t)t * p.dim + (size_t)h * hs;
        float acc = 0.0f;
        for (int i = 0; i < hs; i++) acc = acc + q[i] * k[i];
        s_att[t] = acc / scale_div;
    }
    __syncthreads();
    // softmax_num (cpu.rs:187-192): max, exp(a - max), sum, divide
    float mx = -INFINITY;
    for (int t = tid; t <= pos; t += blockDim.x) mx = fmaxf(mx, s_att[t]);
    mx = block_max(mx, red);
    __syncthreads();
    for (int t = tid; t <= pos; t += blockDim.x) s_att[t] = expf_glibc(s_att[t] - mx);
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        for (int t = 0; t <= pos; t++) sum = sum + s_att[t];
        s_sum = sum;
    }
    __syncthreads();
    const float sum = s_sum;
    for (int t = tid; t <= pos; t += blockDim.x) {
        const float a = s_att[t] / sum;
        s_att[t] = a;
        if (p.att) p.att[(size_t)h * p.seq_len + t] = a;
    }
    __syncthreads();
    for (int i = tid; i < hs; i += blockDim.x) {
        float acc = 0.0f;
        for (int t = 0; t <= pos; t++) acc = acc + s_att[t] * p.vc[(size_t)t * p.dim + (size_t)h * hs + i];
        p.xb[(size_t)h * hs + i] = acc;
    }
}

// ---------------------------------------------------------------- cpu.rs:54-64 sinu, then array_mult
__global__ void sinu_ref_kernel(float* o, size_t n) {
    RAMA_NO_CONTRACT
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float a = o[i];
        o[i] = a * (1.0f / (1.0f + expf_glibc(-a)));
    }
}

// ... followed by Device::array_mult on the same vector (infer.rs:44-45), one launch: the same two roundings per element (cpu.rs:56, :59-64)
__global__ void sinu_mult_ref_kernel(float* o, const float* s, size_t n) {
    RAMA_NO_CONTRACT
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float a = o[i];
        const float g = a * (1.0f / (1.0f + expf_glibc(-a)));
        o[i] = g * s[i];
    }
}

// cpu.rs:119-125 Device::softmax (whole view)
__global__ __launch_bounds__(1024) void softmax_ref_kernel(float* x, int n) {
    RAMA_NO_CONTRACT
    __shared__ float red[16];
    __shared__ float s_sum;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, x[i]);
    mx = block_max(mx, red);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) x[i] = expf_glibc(x[i] - mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.0f;
        for (int i = 0; i < n; i++) sum = sum + x[i];
        s_sum = sum;
    }
    __syncthreads();
    const float sum = s_sum;
    for (int i = threadIdx.x; i < n; i += blockDim.x) x[i] = x[i] / sum;
}

}  // namespace rama
