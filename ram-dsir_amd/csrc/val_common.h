// val_common.h -- what the validation entry points on NCHW fp32 tensors (val_post.hip, val_volume.hip) and their NHWC storage-dtype
// counterparts (infer.hip) share: the validity rules of the host records, the frame chunk that travels in the kernel arguments, and
// the sigmoid -- ONE definition each, so that both layouts accept the same records and form the same bits.
#pragma once
#include "common.h"
#include "../../include/ramdsir.h"

namespace rdval {

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

constexpr int64_t kMaxPixels = 1 << 28;                    // per plane: node indices and areas stay far inside 31 bits
constexpr int64_t kMaxVoxels = 1 << 28;                    // per volume: likewise

inline bool valid_images(const rd_val_image_t* im, int B) {
    if (!im || B < 0) return false;
    for (int i = 0; i < B; ++i)
        if (im[i].h < 1 || im[i].w < 1 || (int64_t)im[i].h * im[i].w > kMaxPixels || im[i].off < 0) return false;
    return true;
}

// every slot empty (-1) or a frame with both neighbours inside the volume; the frames increase, so no two slots write one slice
inline bool valid_frames(const int32_t* f, int B, int D) {
    if (!f || B < 1) return false;
    int last = 0;
    for (int i = 0; i < B; ++i) {
        if (f[i] == -1) continue;
        if (f[i] <= last || f[i] > D - 2) return false;
        last = f[i];
    }
    return true;
}

struct VolFrames {
    int32_t jj[RD_VAL_CHUNK];                               // frame of each slot of the chunk, -1: empty
};

inline VolFrames frames_chunk(const int32_t* f, int b0, int n) {
    VolFrames c;
    for (int i = 0; i < RD_VAL_CHUNK; ++i) c.jj[i] = i < n ? f[b0 + i] : -1;
    return c;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace rdval
