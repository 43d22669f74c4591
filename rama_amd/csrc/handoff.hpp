// handoff.hpp -- the device-side accessors of data handed over INSIDE a launch: the sc1 (write-through / L1-bypassing) loads and stores of
// attn_wo.hpp's counter protocol, and the tagged (value, epoch) words of layer_fused.hpp, which chain.hpp's leader norms use too.  Device
// functions only: chain_api.hip takes them from here and so sees neither attn_wo_kernel nor stage_fused_kernel.
#pragma once
#include "kernels.hpp"

namespace rama {

// ---- sc1 (write-through / L1-bypassing) accessors for inter-workgroup data
__device__ __forceinline__ void st_sc1(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ f4 ld4_sc1(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 16));   // cpol sc1
}

// ---- tagged words: a float and the epoch it was written in, one 8-byte store (the protocol: layer_fused.hpp)
__device__ __forceinline__ void put_tagged(tagged_t* p, float v, unsigned epoch) {
    __hip_atomic_store(p, ((tagged_t)epoch << 32) | (tagged_t)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float get_tagged(const tagged_t* p) {      // a word some phase before the awaited one wrote
    return __uint_as_float((unsigned)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

}  // namespace rama
