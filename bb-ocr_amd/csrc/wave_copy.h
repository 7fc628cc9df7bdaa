// What the one-wavefront decoders of tiffdec.hip and gifdec.hip share: the output policy of tiff_codecs.h / gif_lzw.h for a workgroup of ONE
// wavefront, and the argument why a lane may read what another lane stored.  A lane's global stores are not ordered against another lane's
// later loads by program order alone: drain_and_sync() waits until this wave's stores have left (vmcnt(0)) and then passes the workgroup
// barrier, whose fence lets the loads behind it see them -- with one wavefront per workgroup the barrier costs no waiting.  copy_back
// keeps `synced`, the output position up to which everything was stored before the last drain, and drains again only for a string that
// reaches behind it.  (pngdec.hip's copy_match follows the same rule with a distance instead of a source offset.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

__device__ inline void drain_and_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's stores are out before the barrier's fence lets the others load
    __syncthreads();
}

struct WaveCopy {                                         // a workgroup of ONE wavefront
    static constexpr int kLanes = 64;
    __device__ static void copy_in(uint8_t* out, size_t o, const uint8_t* in, size_t n) {
        for (size_t i = threadIdx.x; i < n; i += kLanes) out[o + i] = in[i];
    }
    __device__ static void fill(uint8_t* out, size_t o, uint8_t v, size_t n) {
        for (size_t i = threadIdx.x; i < n; i += kLanes) out[o + i] = v;
    }
    // out[o .. o + len) = out[src .. src + len); with kwkwk the last byte is the string's first (the entry being defined)
    __device__ static void copy_back(uint8_t* out, size_t o, uint32_t src, uint32_t len, bool kwkwk, size_t& synced) {
        const uint32_t whole = kwkwk ? len - 1 : len;     // these bytes stand before o
        if ((size_t)src + whole > synced) {
            drain_and_sync();
            synced = o;
        }
        for (uint32_t i = threadIdx.x; i < whole; i += kLanes) out[o + i] = out[src + i];
        if (kwkwk && threadIdx.x == 0) out[o + whole] = out[src];
    }
};
