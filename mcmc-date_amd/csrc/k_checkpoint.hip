// k_checkpoint.hip -- the device side of mcd_mh_save / mcd_mh_load (gfx950; ckpt_capi.cpp, ckpt_device.hpp): the handle's arrays and the
// checkpoint blob exchange their 8-byte words in ONE launch each way, in place of some fifteen strided copies with a wait each.
//
//   k_ckpt_pack      blob := the arrays.  The grid covers (section, slab): a workgroup takes kCkptSlab consecutive words of one section, lane
//                    t of pass k word 256 k + t, so a wave stores 512 contiguous bytes and loads them contiguously too (heights and rates:
//                    contiguous inside a row of n_nodes doubles; the int32 counters: two values per word).  Every lane keeps the terms
//                    mix(w XOR (i + 1) golden) of its words, a wave adds them up by shuffles, and its first lane adds the wave's sum to the
//                    section's checksum word with one 64-bit vector atomic: integer addition mod 2^64, so neither the order of the waves
//                    nor the launch geometry can change the word.
//   k_ckpt_verify    the same sums over an uploaded blob's sections, into a small array that the host compares with the section table.
//   k_ckpt_unpack    the arrays := blob, the inverse scatter; launched only after that comparison, so a damaged blob changes nothing.
// All pointers are global memory and are addressed as such (address space 1: global loads and stores, never flat ones).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ckpt_device.hpp"

namespace mcd {

namespace {

enum { PACK = 0, VERIFY = 1, UNPACK = 2 };
typedef __attribute__((address_space(1))) uint64_t g_u64;
typedef __attribute__((address_space(1))) uint32_t g_u32;

// word i of a section, read from / written to the handle's array
__device__ inline uint64_t sec_load(const CkptSec& S, uint64_t i)
{
    if (S.kind == CKPT_ROWS) {
        const uint64_t row = i / (uint64_t)S.row_len, col = i - row * (uint64_t)S.row_len;
        return ((const g_u64*)(uint64_t*)S.arr)[row * (uint64_t)S.ld + col];
    }
    if (S.kind == CKPT_INT32) {
        const g_u32* a = (const g_u32*)(uint32_t*)S.arr;
        const uint64_t lo = a[2 * i], hi = (2 * i + 1 < (uint64_t)S.row_len) ? a[2 * i + 1] : 0u;
        return lo | hi << 32;
    }
    return ((const g_u64*)(uint64_t*)S.arr)[i];
}

__device__ inline void sec_store(const CkptSec& S, uint64_t i, uint64_t w)
{
    if (S.kind == CKPT_ROWS) {
        const uint64_t row = i / (uint64_t)S.row_len, col = i - row * (uint64_t)S.row_len;
        ((g_u64*)(uint64_t*)S.arr)[row * (uint64_t)S.ld + col] = w;
    } else if (S.kind == CKPT_INT32) {
        g_u32* a = (g_u32*)(uint32_t*)S.arr;
        a[2 * i] = (uint32_t)w;
        if (2 * i + 1 < (uint64_t)S.row_len) a[2 * i + 1] = (uint32_t)(w >> 32);
    } else
        ((g_u64*)(uint64_t*)S.arr)[i] = w;
}

template <int MODE>
__device__ inline void ckpt_body(const CkptJob& J)
{
    const unsigned blk = blockIdx.x;
    int s = 0;
    for (int k = 1; k < J.n; ++k)
        if (blk >= J.s[k].first_block) s = k;              // (uniform: the sections' first workgroups ascend)
    const CkptSec S = J.s[s];
    g_u64* blob = (g_u64*)J.blob + S.blob_word;
    const uint64_t base = (uint64_t)(blk - S.first_block) * kCkptSlab;
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kCkptSlab / 256; ++k) {
        const uint64_t i = base + (uint64_t)(k * 256) + threadIdx.x;
        if (i >= S.n_words) break;
        uint64_t w;
        if (MODE == PACK) {
            w = sec_load(S, i);
            blob[i] = w;
        } else {
            w = blob[i];
            if (MODE == UNPACK) sec_store(S, i, w);
        }
        if (MODE != UNPACK) sum += ckpt_mix(w ^ ((i + 1) * 0x9E3779B97F4A7C15ULL));
    }
    if (MODE != UNPACK) {
        for (int d = 32; d >= 1; d >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, d, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(J.sums + (size_t)s * J.sum_stride, (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(256) void k_ckpt_pack(CkptJob J) { ckpt_body<PACK>(J); }
__global__ __launch_bounds__(256) void k_ckpt_verify(CkptJob J) { ckpt_body<VERIFY>(J); }
__global__ __launch_bounds__(256) void k_ckpt_unpack(CkptJob J) { ckpt_body<UNPACK>(J); }

template <int MODE>
hipError_t launch(const CkptJob& J, unsigned blocks, hipStream_t st)
{
    if (J.n < 1 || J.n > kCkptMaxSections || J.blob == nullptr || (MODE != UNPACK && J.sums == nullptr)) return hipErrorInvalidValue;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(MODE == PACK ? k_ckpt_pack : MODE == VERIFY ? k_ckpt_verify : k_ckpt_unpack, dim3(blocks), dim3(256), 0, st, J);
    return hipGetLastError();
}

}  // namespace

bool ckpt_plan(CkptJob* J, unsigned* blocks)
{
    uint64_t b = 0;
    for (int s = 0; s < J->n; ++s) {
        J->s[s].first_block = (unsigned)b;
        b += (J->s[s].n_words + kCkptSlab - 1) / kCkptSlab;
        if (b > 0x7fffffffULL) return false;
    }
    *blocks = (unsigned)b;
    return true;
}

hipError_t launch_ckpt_pack(const CkptJob& J, unsigned blocks, hipStream_t st) { return launch<PACK>(J, blocks, st); }
hipError_t launch_ckpt_verify(const CkptJob& J, unsigned blocks, hipStream_t st) { return launch<VERIFY>(J, blocks, st); }
hipError_t launch_ckpt_unpack(const CkptJob& J, unsigned blocks, hipStream_t st) { return launch<UNPACK>(J, blocks, st); }

}  // namespace mcd
