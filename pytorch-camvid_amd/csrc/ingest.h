#pragma once
// ingest.h: image ingest.  uint8 frames to normalised float32 NHWC (cvk_preprocess_u8) and the fused train / val transform of a batch of
// frames and masks from one record per image (cvk_augment_u8, cvk_augment_record_bytes).  crop_aug.h is included for the pieces of the
// resampling that it holds once for both transforms (aug_reflect101, aug_round_u8, aug_coord).
#include "cvk_common.h"
#include "crop_aug.h"

namespace {

// uint8 HWC (cv2 BGR order kept) -> float32 NHWC, 4 channels per pixel (3 valid + zero pad): (v/255 - mean[c]) / std[c]
// = reference transforms.ToTensor + Normalize (transforms.py:485-538) with conf/settings.py:8-9 MEAN/STD passed in.
__global__ void k_preprocess_u8(const uint8_t* __restrict__ src, float* __restrict__ dst, long npix, float m0, float m1,
                                float m2, float r0, float r1, float r2) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
        const uint8_t* p = src + i * 3;
        f32x4 v;
        v[0] = ((float)p[0] * (1.f / 255.f) - m0) * r0;
        v[1] = ((float)p[1] * (1.f / 255.f) - m1) * r1;
        v[2] = ((float)p[2] * (1.f / 255.f) - m2) * r2;
        v[3] = 0.f;
        *reinterpret_cast<f32x4*>(dst + i * 4) = v;
    }
}

// The reference's train / val transforms (transforms.py Resize -> RandomGaussianBlur -> RandomHorizontalFlip -> ColorJitter ->
// ToTensor -> Normalize, train.py:61-75) fused: a workgroup owns one AUG_TW x AUG_TH output tile of one image (grid x, y, N).
// Stage A resamples the tile plus a blur halo of R = (ksize-1)/2 pixels (REFLECT_101 in resized coordinates, cv2.GaussianBlur's
// default border) bilinearly from the source frame into LDS, rounded to uint8 values; stage B runs the separable Gaussian
// (horizontal into s_h, then vertical, fp32), rounds, applies the LUT and normalises with k_preprocess_u8's expression; the flip
// is applied at the store (the blur is symmetric and the LUT per pixel, so both commute with it).  R is uniform per image
// (blockIdx.z), hence a template argument chosen by one uniform switch.
constexpr int AUG_TW = 64, AUG_TH = 16, AUG_RMAX = 4;
constexpr int AUG_LW = AUG_TW + 2 * AUG_RMAX, AUG_LH = AUG_TH + 2 * AUG_RMAX;

struct AugArgs {
    const uint8_t* frames;
    const void* masks;
    int mask_bytes, Hs, Ws, H, W;
    double sy, sx;                      // Hs / H, Ws / W (cv2 computes both mappings in double)
    const cvk_augment_record* records;
    float m0, m1, m2, r0, r1, r2;
    float* out;
    int64_t* out_masks;
    uint8_t* out_u8;
};

// aug_reflect101, aug_round_u8 and aug_coord: crop_aug.h

template <int R>
__device__ __forceinline__ void aug_tile(const AugArgs& A, const cvk_augment_record* rec, float* s_in, float* s_h,
                                         const uint8_t* s_lut, bool use_lut) {
    constexpr int LWr = AUG_TW + 2 * R, LHr = AUG_TH + 2 * R;
    const int n = blockIdx.z, x0 = blockIdx.x * AUG_TW, y0 = blockIdx.y * AUG_TH;
    const uint8_t* src = A.frames + (size_t)n * A.Hs * A.Ws * 3;

    // stage A: resized uint8 values of the tile and its halo -> s_in[c][ly][lx] (row stride AUG_LW)
    for (int idx = threadIdx.x; idx < LHr * LWr; idx += blockDim.x) {
        const int ly = idx / LWr, lx = idx - ly * LWr;
        const int ry = aug_reflect101(y0 - R + ly, A.H), rx = aug_reflect101(x0 - R + lx, A.W);
        int iy0, iy1, ix0, ix1;
        float ay, ax;
        aug_coord(ry, A.sy, A.Hs, iy0, iy1, ay);
        aug_coord(rx, A.sx, A.Ws, ix0, ix1, ax);
        const uint8_t* p00 = src + ((size_t)iy0 * A.Ws + ix0) * 3;
        const uint8_t* p01 = src + ((size_t)iy0 * A.Ws + ix1) * 3;
        const uint8_t* p10 = src + ((size_t)iy1 * A.Ws + ix0) * 3;
        const uint8_t* p11 = src + ((size_t)iy1 * A.Ws + ix1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = (1.f - ax) * (float)p00[c] + ax * (float)p01[c];
            const float bot = (1.f - ax) * (float)p10[c] + ax * (float)p11[c];
            s_in[(c * AUG_LH + ly) * AUG_LW + lx] = aug_round_u8((1.f - ay) * top + ay * bot);
        }
    }
    float tp[2 * R + 1];
#pragma unroll
    for (int t = 0; t < 2 * R + 1; ++t) tp[t] = rec->taps[t];
    __syncthreads();

    if (R > 0) {  // horizontal pass over every staged row -> s_h[c][ly][tx] (row stride AUG_TW)
        for (int idx = threadIdx.x; idx < LHr * AUG_TW; idx += blockDim.x) {
            const int ly = idx / AUG_TW, tx = idx - ly * AUG_TW;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* row = s_in + (c * AUG_LH + ly) * AUG_LW + tx;
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 2 * R + 1; ++t) acc = fmaf(tp[t], row[t], acc);
                s_h[(c * AUG_LH + ly) * AUG_TW + tx] = acc;
            }
        }
        __syncthreads();
    }

    const bool flip = rec->flip != 0;
    for (int idx = threadIdx.x; idx < AUG_TH * AUG_TW; idx += blockDim.x) {
        const int ty = idx / AUG_TW, tx = idx - ty * AUG_TW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= A.H || x >= A.W) continue;
        float u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v;
            if (R > 0) {
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 2 * R + 1; ++t) acc = fmaf(tp[t], s_h[(c * AUG_LH + ty + t) * AUG_TW + tx], acc);
                v = aug_round_u8(acc);
            } else {
                v = s_in[(c * AUG_LH + ty) * AUG_LW + tx];
            }
            u[c] = use_lut ? (float)s_lut[(int)v] : v;
        }
        const int xo = flip ? A.W - 1 - x : x;
        const size_t o = ((size_t)n * A.H + y) * A.W + xo;
        f32x4 f;
        f[0] = (u[0] * (1.f / 255.f) - A.m0) * A.r0;
        f[1] = (u[1] * (1.f / 255.f) - A.m1) * A.r1;
        f[2] = (u[2] * (1.f / 255.f) - A.m2) * A.r2;
        f[3] = 0.f;
        *reinterpret_cast<f32x4*>(A.out + o * 4) = f;
        if (A.out_u8) {
            A.out_u8[o * 3 + 0] = (uint8_t)u[0];
            A.out_u8[o * 3 + 1] = (uint8_t)u[1];
            A.out_u8[o * 3 + 2] = (uint8_t)u[2];
        }
        // mask: cv2 INTER_NEAREST, source floor(d * in / out) in double, clamped to the last row / column
        const int my = min((int)floor(y * A.sy), A.Hs - 1), mx = min((int)floor(x * A.sx), A.Ws - 1);
        const size_t mi = ((size_t)n * A.Hs + my) * A.Ws + mx;
        A.out_masks[o] = A.mask_bytes == 1 ? (int64_t)static_cast<const uint8_t*>(A.masks)[mi] : static_cast<const int64_t*>(A.masks)[mi];
    }
}

__global__ void __launch_bounds__(256) k_augment_u8(AugArgs A) {
    __shared__ float s_in[3 * AUG_LH * AUG_LW];
    __shared__ float s_h[3 * AUG_LH * AUG_TW];
    __shared__ uint8_t s_lut[256];
    const cvk_augment_record* rec = A.records + blockIdx.z;
    const bool use_lut = rec->use_lut != 0;
    if (use_lut)
        for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lut[i] = rec->lut[i];   // visible after stage A's barrier
    const int k = rec->ksize;
    const int r = (k == 3 || k == 5 || k == 7 || k == 9) ? (k - 1) / 2 : 0;
    switch (r) {
        case 0: aug_tile<0>(A, rec, s_in, s_h, s_lut, use_lut); break;
        case 1: aug_tile<1>(A, rec, s_in, s_h, s_lut, use_lut); break;
        case 2: aug_tile<2>(A, rec, s_in, s_h, s_lut, use_lut); break;
        case 3: aug_tile<3>(A, rec, s_in, s_h, s_lut, use_lut); break;
        default: aug_tile<4>(A, rec, s_in, s_h, s_lut, use_lut); break;
    }
}

}  // namespace

extern "C" int cvk_augment_record_bytes(void) { return (int)sizeof(cvk_augment_record); }

extern "C" int cvk_augment_u8(const uint8_t* frames, const void* masks, int mask_bytes, int N, int Hs, int Ws, int H, int W,
                              const cvk_augment_record* records, const float* mean3, const float* std3, float* out,
                              int64_t* out_masks, uint8_t* out_u8, void* stream) {
    CVK_CHECK_ARG(frames && masks && records && mean3 && std3 && out && out_masks, "cvk_augment_u8: null pointer");
    CVK_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && (mask_bytes == 1 || mask_bytes == 8) && cvk_aligned16(out),
                  "cvk_augment_u8: bad arguments");
    CVK_CHECK_ARG(N <= 65535 && cvk_cdiv(H, AUG_TH) <= 65535, "cvk_augment_u8: grid too large");
    CVK_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "cvk_augment_u8: zero std");
    AugArgs a;
    a.frames = frames; a.masks = masks; a.mask_bytes = mask_bytes;
    a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
    a.sy = (double)Hs / H; a.sx = (double)Ws / W;
    a.records = records;
    a.m0 = mean3[0]; a.m1 = mean3[1]; a.m2 = mean3[2];
    a.r0 = 1.f / std3[0]; a.r1 = 1.f / std3[1]; a.r2 = 1.f / std3[2];
    a.out = out; a.out_masks = out_masks; a.out_u8 = out_u8;
    hipLaunchKernelGGL(k_augment_u8, dim3(cvk_cdiv(W, AUG_TW), cvk_cdiv(H, AUG_TH), N), dim3(256), 0, (hipStream_t)stream, a);
    CVK_LAUNCH_RETURN("cvk_augment_u8");
}

extern "C" int cvk_preprocess_u8(const uint8_t* src, float* dst, int N, int H, int W, const float* mean3, const float* std3,
                                 void* stream) {
    CVK_CHECK_ARG(src && dst && mean3 && std3 && N > 0 && H > 0 && W > 0 && cvk_aligned16(dst), "cvk_preprocess_u8: bad arguments");
    CVK_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "cvk_preprocess_u8: zero std");
    const long npix = (long)N * H * W;
    const long b = (npix + 255) / 256;
    hipLaunchKernelGGL(k_preprocess_u8, dim3((int)(b < 8192 ? b : 8192)), dim3(256), 0, (hipStream_t)stream, src, dst, npix, mean3[0],
                       mean3[1], mean3[2], 1.f / std3[0], 1.f / std3[1], 1.f / std3[2]);
    CVK_LAUNCH_RETURN("cvk_preprocess_u8");
}
