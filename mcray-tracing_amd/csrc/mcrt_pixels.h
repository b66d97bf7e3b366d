// mcrt_pixels.h -- the pixel tile of the kernels that gather an image stack through cached maps into pictures (k_bmode and k_compound in
// mcrt_display.hip, k_volume, k_label_gather; k_render takes the byte alone): which points a lane owns, which frames a workgroup walks,
// the persistence step, what a displayed byte is, and how a wavefront's values leave.  A PixelPass (mcrt_kernels.h) describes the pass.
// THE LAYOUT (measured, DESIGN 5.7: which points a lane owns decides the speed).  A workgroup is four wavefronts; a wavefront owns 256
// consecutive points from wb on, a lane the four points wb + 64 j + lane, j = 0..3: in every gather instruction the 64 lanes ask for 64
// NEIGHBOURING points, as k_remap's do.  The maps are padded to n_pad, a multiple of 256 points, with zeros: a lane reads its four map
// values without a test (p0 + 192 < n_pad), the points past the picture's end read tap (0, 0), which exists, and are not stored.
// blockIdx.y is a chunk of frames_per_chunk frames [f0, f1); the last chunk may be short.  Floats leave as they are, 256 contiguous bytes
// per instruction.  Bytes are first turned round: byte j of a lane is point wb + 64 j + lane, and four ds_bpermute give lane L the bytes of
// the points wb + 4 L .. 4 L + 3, one aligned word -- where pass.vec says that n % 4 == 0 and the output is word-aligned, and the wavefront
// is whole (every lane is active); a wavefront at the picture's end, or any wavefront without pass.vec, stores its bytes one by one.
#pragma once
#include "mcrt_device.h"

namespace mcrt {

// the launch of a pass: 1024 points per workgroup of 256 lanes, one chunk of frames per blockIdx.y.  (k_bmode's lanes own 4 consecutive
// points each: its ((n + 3) / 4 + 255) / 256 workgroups are the same (n + 1023) / 1024.)
inline dim3 pixel_grid(const PixelPass &p) { return dim3((p.n + 1023u) / 1024u, (p.F + p.frames_per_chunk - 1u) / p.frames_per_chunk); }
struct PixelTile { uint32_t lane, wb, p0, f0, f1; bool whole; };      // p0 = wb + lane: the lane's points are p0 + 64 j; whole: all 256 points are inside n
// the frames [f0, f1) of this workgroup's chunk
MCRT_DEV void frame_window(const PixelPass &p, uint32_t &f0, uint32_t &f1) { f0 = blockIdx.y * p.frames_per_chunk; f1 = min(p.F, f0 + p.frames_per_chunk); }
// false: the whole wavefront lies past the picture's end and leaves
MCRT_DEV bool pixel_tile(const PixelPass &p, PixelTile &t)
{
    t.lane = threadIdx.x & 63u; t.wb = blockIdx.x * 1024u + (threadIdx.x >> 6) * 256u; t.p0 = t.wb + t.lane;
    t.whole = t.wb + 256u <= p.n;
    frame_window(p, t.f0, t.f1);
    return t.wb < p.n;
}
// what a displayed byte is: y in [0, 1] -> 0 .. 255, rounded to nearest
MCRT_DEV uint8_t quantise(float y) { return (uint8_t)(y * 255.0f + 0.5f); }
MCRT_DEV uint32_t quantise4(const float (&y)[4])                      // byte j: y[j]
{
    uint32_t bytes = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) bytes |= (uint32_t)quantise(y[j]) << (8 * j);
    return bytes;
}
// one frame's four values of a lane leave (out_frame: the frame's first point)
MCRT_DEV void tile_store_f32(float *out_frame, const PixelTile &t, uint32_t n, const float (&v)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) if (t.p0 + 64u * j < n) out_frame[t.p0 + 64u * j] = v[j];
}
MCRT_DEV void tile_store_u8(uint8_t *out_frame, const PixelTile &t, uint32_t n, uint32_t bytes, bool word_ok)
{
    if (word_ok && t.whole) {                       // point wb + 4 L + i is byte L / 16 of lane (4 L + i) % 64
        uint32_t word = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((4u * t.lane + (uint32_t)i) & 63u) * 4u), (int)bytes);
            word |= ((got >> (8u * (t.lane >> 4))) & 0xffu) << (8 * i);
        }
        *(uint32_t *)(out_frame + t.wb + 4u * t.lane) = word;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) if (t.p0 + 64u * j < n) out_frame[t.p0 + 64u * j] = (uint8_t)(bytes >> (8 * j));
    }
}
// Persistence (step 5 of mcrt_bmode_frames) as a register recurrence over the frames a lane walks: y = fmaf(alpha, y_prev, (1 - alpha) * s),
// y = s for the first frame after a reset and without persistence (smooth = alpha > 0 is false).  The lane's four points are p0 + stride j
// (k_bmode: stride 1, k_compound: 64); their state is read before the first frame (true: there is a y_prev).  The kernels write it back themselves
// after the pass's last frame (f1 == F): as a function here, that store cost k_compound's max 8-bit forms 3 registers (profiles/pixel_tile).
MCRT_DEV bool persist_load(float (&y)[4], bool smooth, const float *state, uint32_t reset, uint32_t p0, uint32_t stride, uint32_t n)
{
#pragma unroll
    for (int j = 0; j < 4; j++) y[j] = 0.0f;
    if (!(smooth && state && !reset)) return false;
#pragma unroll
    for (int j = 0; j < 4; j++) y[j] = p0 + stride * j < n ? state[p0 + stride * j] : 0.0f;
    return true;
}
MCRT_DEV void persist_step(float (&y)[4], bool &have_prev, bool smooth, float alpha, const float (&v)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) y[j] = !smooth ? v[j] : fmaf(alpha, have_prev ? y[j] : v[j], (1.0f - alpha) * v[j]);
    have_prev = true;
}

}  // namespace mcrt
