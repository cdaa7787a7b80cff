// GPU input pipeline: the reference's per-sample torchvision transforms
// (notebooks/train_multimodal_fusion.py:172-205) on a decoded batch, bit-exact with the PIL
// backend torchvision drives for PIL images.  The host only decodes (PIL, as the reference's
// DataLoader workers do) and packs bytes; everything after decode runs here:
//   Resize((224, 224))            PIL Image.resize(BILINEAR): separable antialiased resample,
//                                 22-bit fixed-point taps, horizontal pass then vertical, each
//                                 rounded to u8 (k_resize_h, k_resize_v; taps from
//                                 dfu_resize_coeffs on the host)
//   standardize_images.py         the reference's offline letterbox (scripts/standardize_images.py:
//                                 58-76) in place of the Resize: the same two passes with each
//                                 image's own out_w x out_h, written at (pad_x, pad_y) of a black
//                                 T x T canvas (k_letterbox_h, k_letterbox_v: the second pass
//                                 writes box and border, every byte once; dfu_letterbox_batch)
//   Random{Horizontal,Vertical}Flip, RandomRotation(30), ColorJitter(0.3, 0.3, 0.3),
//   RandomAffine(20, (0.1, 0.1), (0.8, 1.2)), ToTensor, Normalize
//                                 one gather kernel per output pixel (k_augment_apply): PIL's
//                                 16.16 fixed-point nearest-neighbour affine maps (fill 0), the
//                                 ImageEnhance blends in fp32 with truncation, /255 and the
//                                 normalisation in fp32 with IEEE division -> fp32 NCHW
//   ImageEnhance.Contrast needs the mean grey level of the image it is applied to: one block
//   per image reduces it first (k_augment_stats).
//   GaussianBlur(3, sigma)        the thermal-only script's last random op
//                                 (notebooks/train_thermal_only.py:103-112), between RandomAffine
//                                 and ToTensor: torchvision F.gaussian_blur on the u8 image,
//                                 reflect pad 1, nine fp32 taps, round half to even
//                                 (k_augment_blur in place of k_augment_apply: an LDS tile of
//                                 pre-blur pixels with halo; dfu_augment_blur).  Restated from
//                                 torchvision's source, parity unpinned (dfu_hip.h).
// Random parameters are drawn on the host (data/gpu_transforms.py) and arrive per image as
// dfu_aug_params; all arithmetic here is integer except the blends and the normalisation.
// Test-time augmentation (notebooks/test_time_augmentation.py:145-167) uses the same two kernels
// through dfu_augment_views: K outputs gathered from one resized image (view_src), and the TTA
// Compose's order, rotation before the flips.
#include <cmath>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)  // the blends and the normalisation round like the CPU code

namespace {

constexpr int kPrec = 22;  // PIL Resample.c PRECISION_BITS (32 - 8 - 2)
constexpr int TPB = 256;

DFU_DEV int clip8(int s) {
  const int v = s >> kPrec;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Horizontal pass: tmp[img][y][x] for every source row y, out width OW; one thread per output
// pixel, the source bytes through L1/L2 (a wave-per-row LDS-staged variant measured 1.6x
// slower: its load and compute phases do not overlap at the occupancy its LDS allows).
__global__ void k_resize_h(const uint8_t* __restrict__ src, const dfu_resize_desc* __restrict__ d,
                           const int32_t* __restrict__ coefs, int OW, uint8_t* __restrict__ tmp) {
  const dfu_resize_desc D = d[blockIdx.y];
  const int32_t* bnd = coefs + D.coef_off;
  const int32_t* kk = bnd + 2 * OW;
  const int64_t n = (int64_t)D.h * OW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / OW), x = (int)(i % OW);
    const int xmin = bnd[2 * x], cnt = bnd[2 * x + 1];
    const int32_t* k = kk + (int64_t)x * D.ksh;
    const uint8_t* p = src + D.src_off + ((int64_t)y * D.w + xmin) * 3;
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < cnt; ++j) {
      const int w = k[j];
      s0 += p[3 * j] * w;
      s1 += p[3 * j + 1] * w;
      s2 += p[3 * j + 2] * w;
    }
    uint8_t* o = tmp + D.tmp_off + i * 3;
    o[0] = (uint8_t)clip8(s0);
    o[1] = (uint8_t)clip8(s1);
    o[2] = (uint8_t)clip8(s2);
  }
}

// Vertical pass over the horizontal result: dst[img][y][x][3], OH x OW.
__global__ void k_resize_v(const uint8_t* __restrict__ tmp, const dfu_resize_desc* __restrict__ d,
                           const int32_t* __restrict__ coefs, int OW, int OH,
                           uint8_t* __restrict__ dst) {
  const dfu_resize_desc D = d[blockIdx.y];
  const int32_t* bnd = coefs + D.coef_off + 2 * OW + (int64_t)OW * D.ksh;
  const int32_t* kk = bnd + 2 * OH;
  const int n = OH * OW;
  uint8_t* out = dst + (int64_t)blockIdx.y * n * 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int y = i / OW, x = i % OW;
    const int ymin = bnd[2 * y], cnt = bnd[2 * y + 1];
    const int32_t* k = kk + (int64_t)y * D.ksv;
    const uint8_t* p = tmp + D.tmp_off + ((int64_t)ymin * OW + x) * 3;
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < cnt; ++j) {
      const int w = k[j];
      const uint8_t* q = p + (int64_t)j * OW * 3;
      s0 += q[0] * w;
      s1 += q[1] * w;
      s2 += q[2] * w;
    }
    out[i * 3] = (uint8_t)clip8(s0);
    out[i * 3 + 1] = (uint8_t)clip8(s1);
    out[i * 3 + 2] = (uint8_t)clip8(s2);
  }
}

// Letterbox (dfu_letterbox_batch): the two passes above with per-image output sizes.  boxes:
// int32 [n][4] = out_w, out_h, pad_x, pad_y.
constexpr int kBoxW = 0, kBoxH = 1, kBoxX = 2, kBoxY = 3;

// One output pixel of a pass: cnt taps k over the source pixels p, p + stride, ...
DFU_DEV void tap_sum(const uint8_t* p, int64_t stride, const int32_t* k, int cnt, uint8_t* o) {
  int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
  for (int j = 0; j < cnt; ++j) {
    const int w = k[j];
    const uint8_t* q = p + j * stride;
    s0 += q[0] * w;
    s1 += q[1] * w;
    s2 += q[2] * w;
  }
  o[0] = (uint8_t)clip8(s0);
  o[1] = (uint8_t)clip8(s1);
  o[2] = (uint8_t)clip8(s2);
}

// k_resize_h with the image's own output width: tmp[img][y][x], h x out_w.
__global__ void k_letterbox_h(const uint8_t* __restrict__ src,
                              const dfu_resize_desc* __restrict__ d,
                              const int32_t* __restrict__ boxes,
                              const int32_t* __restrict__ coefs, uint8_t* __restrict__ tmp) {
  const dfu_resize_desc D = d[blockIdx.y];
  const int OW = boxes[4 * blockIdx.y + kBoxW];
  const int32_t* bnd = coefs + D.coef_off;
  const int32_t* kk = bnd + 2 * OW;
  const int64_t n = (int64_t)D.h * OW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / OW), x = (int)(i % OW);
    tap_sum(src + D.src_off + ((int64_t)y * D.w + bnd[2 * x]) * 3, 3, kk + (int64_t)x * D.ksh,
            bnd[2 * x + 1], tmp + D.tmp_off + i * 3);
  }
}

// Vertical pass onto the T x T canvas: one thread per canvas pixel, which is either a pixel of
// the box (the vertical taps over tmp) or border (0); every byte of dst is written once.
__global__ void k_letterbox_v(const uint8_t* __restrict__ tmp,
                              const dfu_resize_desc* __restrict__ d,
                              const int32_t* __restrict__ boxes,
                              const int32_t* __restrict__ coefs, int T,
                              uint8_t* __restrict__ dst) {
  const dfu_resize_desc D = d[blockIdx.y];
  const int32_t* box = boxes + 4 * blockIdx.y;
  const int OW = box[kBoxW], OH = box[kBoxH], px = box[kBoxX], py = box[kBoxY];
  const int32_t* bnd = coefs + D.coef_off + 2 * OW + (int64_t)OW * D.ksh;
  const int32_t* kk = bnd + 2 * OH;
  const int n = T * T;
  uint8_t* out = dst + (int64_t)blockIdx.y * n * 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int y = i / T - py, x = i % T - px;
    uint8_t* o = out + (int64_t)i * 3;
    if (x >= 0 && x < OW && y >= 0 && y < OH) {
      tap_sum(tmp + D.tmp_off + ((int64_t)bnd[2 * y] * OW + x) * 3, (int64_t)OW * 3,
              kk + (int64_t)y * D.ksv, bnd[2 * y + 1], o);
    } else {
      o[0] = o[1] = o[2] = 0;
    }
  }
}

struct Px {
  int c[3];
};

// PIL Geometry.c affine_fixed: source = ((a2 + y*a1 + x*a0) >> 16, (a5 + y*a4 + x*a3) >> 16).
DFU_DEV bool affine_src(const int32_t* a, int x, int y, int W, int H, int& xs, int& ys) {
  xs = (a[2] + y * a[1] + x * a[0]) >> 16;
  ys = (a[5] + y * a[4] + x * a[3]) >> 16;
  return xs >= 0 && xs < W && ys >= 0 && ys < H;
}

// The resized image after its flips and rotation, at (x, y); rotation fill is black.  ORDER is
// the Compose's: DFU_AUG_ORDER_FLIP_ROTATE flips first (the train scripts), so the inverse chain
// is rotation map -> un-flip -> fetch; DFU_AUG_ORDER_ROTATE_FLIP rotates first (the TTA script),
// so it is un-flip -> rotation map -> fetch.
template <int ORDER>
DFU_DEV Px rotated(const uint8_t* im, const dfu_aug_params& P, int W, int H, int x, int y) {
  Px p = {{0, 0, 0}};
  if (ORDER == DFU_AUG_ORDER_ROTATE_FLIP) {
    if (P.hflip) x = W - 1 - x;
    if (P.vflip) y = H - 1 - y;
  }
  if (P.rotate && !affine_src(P.rot, x, y, W, H, x, y)) return p;
  if (ORDER == DFU_AUG_ORDER_FLIP_ROTATE) {
    if (P.hflip) x = W - 1 - x;
    if (P.vflip) y = H - 1 - y;
  }
  const uint8_t* q = im + ((int64_t)y * W + x) * 3;
  p.c[0] = q[0];
  p.c[1] = q[1];
  p.c[2] = q[2];
  return p;
}

// PIL Convert.c rgb2l: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
DFU_DEV int grey(const Px& p) { return (p.c[0] * 19595 + p.c[1] * 38470 + p.c[2] * 7471 + 0x8000) >> 16; }

// PIL ImagingBlend(degenerate, image, alpha): float(in1) + alpha * float(in2 - in1), clipped
// to [0, 255] and truncated.
DFU_DEV int blend(int in1, int in2, float alpha) {
  const float t = (float)in1 + alpha * (float)(in2 - in1);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// ColorJitter ops [0, upto) in their drawn order; `mean` is the contrast op's grey mean.
DFU_DEV Px colour(Px p, const dfu_aug_params& P, int upto, int mean) {
  for (int k = 0; k < upto; ++k) {
    const float f = P.factor[k];
    if (f == 1.f) continue;  // ImagingBlend copies the image for alpha == 1
    int deg[3];
    if (P.op[k] == DFU_AUG_BRIGHTNESS) {
      deg[0] = deg[1] = deg[2] = 0;
    } else if (P.op[k] == DFU_AUG_CONTRAST) {
      deg[0] = deg[1] = deg[2] = mean;
    } else {
      deg[0] = deg[1] = deg[2] = grey(p);
    }
    if (f == 0.f) {
      for (int c = 0; c < 3; ++c) p.c[c] = deg[c];
    } else {
      for (int c = 0; c < 3; ++c) p.c[c] = blend(deg[c], p.c[c], f);
    }
  }
  return p;
}

DFU_DEV int contrast_slot(const dfu_aug_params& P) {
  for (int k = 0; k < P.n_ops; ++k)
    if (P.op[k] == DFU_AUG_CONTRAST) return k;
  return -1;
}

// ImageEnhance.Contrast needs int(mean(L) + 0.5) of the image entering the contrast op:
// kStatBlocks blocks per image add their grey sums into sums[img] (integer atomics: the
// order does not matter).  sum <= 255 * H * W fits int32 for H * W < 8.4M.
constexpr int kStatBlocks = 8;

// Output image v reads resized image view_src[v] (v itself without view_src); -1 for an index
// outside [0, n_images), whose output is the fill.
DFU_DEV int view_image(const int32_t* view_src, int v, int n_images) {
  const int s = view_src ? view_src[v] : v;
  return s >= 0 && s < n_images ? s : -1;
}

template <int ORDER>
__global__ void __launch_bounds__(256) k_augment_stats(const uint8_t* __restrict__ img,
                                                       const dfu_aug_params* __restrict__ params,
                                                       const int32_t* __restrict__ view_src,
                                                       int n_images, int H, int W,
                                                       int32_t* __restrict__ sums) {
  const dfu_aug_params P = params[blockIdx.y];
  const int slot = contrast_slot(P);
  const int src = view_image(view_src, blockIdx.y, n_images);
  if (slot < 0 || src < 0) return;
  const uint8_t* im = img + (int64_t)src * H * W * 3;
  int s = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * W; i += gridDim.x * blockDim.x) {
    const Px p = colour(rotated<ORDER>(im, P, W, H, i % W, i / W), P, slot, 0);
    s += grey(p);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(sums + blockIdx.y, s);
}

template <int ORDER>
__global__ void k_augment_apply(const uint8_t* __restrict__ img,
                                const dfu_aug_params* __restrict__ params,
                                const int32_t* __restrict__ view_src, int n_images,
                                const int32_t* __restrict__ means, int H, int W, float m0, float m1,
                                float m2, float s0, float s1, float s2, float* __restrict__ out) {
  const dfu_aug_params P = params[blockIdx.y];
  const int src = view_image(view_src, blockIdx.y, n_images);
  const uint8_t* im = img + (int64_t)(src < 0 ? 0 : src) * H * W * 3;
  const int n = H * W;
  // == int(sum / n + 0.5), ImageStat's mean rounded as ImageEnhance.Contrast does
  const int mean = contrast_slot(P) >= 0 ? (int)((2 * (int64_t)means[blockIdx.y] + n) / (2 * (int64_t)n)) : 0;
  float* o = out + (int64_t)blockIdx.y * 3 * n;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int x = i % W, y = i / W;
    Px p = {{0, 0, 0}};
    if (src >= 0 && (!P.affine || affine_src(P.aff, x, y, W, H, x, y)))
      p = colour(rotated<ORDER>(im, P, W, H, x, y), P, P.n_ops, mean);
    o[i] = ((float)p.c[0] / 255.f - m0) / s0;
    o[n + i] = ((float)p.c[1] / 255.f - m1) / s1;
    o[2 * n + i] = ((float)p.c[2] / 255.f - m2) / s2;
  }
}

// The two launches behind dfu_augment_normalize (view_src NULL: image v -> output v) and
// dfu_augment_views.
template <int ORDER>
int launch_augment(const uint8_t* img, const dfu_aug_params* params, const int32_t* view_src,
                   int n_images, int n_out, int H, int W, const float* mean3, const float* std3,
                   int32_t* contrast_means, float* out, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(contrast_means, 0, sizeof(int32_t) * n_out, stream);
  DFU_CHECK_ARG(e == hipSuccess, "augment: memset: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_augment_stats<ORDER>, dim3(kStatBlocks, n_out), dim3(256), 0, stream, img,
                     params, view_src, n_images, H, W, contrast_means);
  DFU_LAUNCH_CHECK();
  const int gx = (H * W + TPB - 1) / TPB;
  hipLaunchKernelGGL(k_augment_apply<ORDER>, dim3(gx < 64 ? gx : 64, n_out), dim3(TPB), 0, stream,
                     img, params, view_src, n_images, contrast_means, H, W, mean3[0], mean3[1],
                     mean3[2], std3[0], std3[1], std3[2], out);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}

// GaussianBlur(kernel_size=3) after the ops above (the thermal-only train transform).  One block
// produces a kBlurTW x kBlurTH tile: it first stages the tile's pre-blur pixels (what
// k_augment_apply computes at that position) plus a 1-pixel halo in LDS, u8 x 3 packed in a
// dword, so the inverse maps and the blends run once per pixel and not once per tap.  The halo
// reflects about the edge of the augmented image (-1 -> 1, W -> W - 2) before the inverse
// chain, so rotation / affine fill is blurred into its neighbours.  A 32-lane half reads 32
// consecutive dwords of one LDS row for every tap and the staging stores are consecutive too:
// no bank conflicts at the unpadded row stride.
constexpr int kBlurTW = 32, kBlurTH = 8;
constexpr int kBlurLW = kBlurTW + 2, kBlurLH = kBlurTH + 2;

template <int ORDER>
DFU_DEV Px augmented(const uint8_t* im, const dfu_aug_params& P, int src, int W, int H, int mean,
                     int x, int y) {
  Px p = {{0, 0, 0}};
  if (src >= 0 && (!P.affine || affine_src(P.aff, x, y, W, H, x, y)))
    p = colour(rotated<ORDER>(im, P, W, H, x, y), P, P.n_ops, mean);
  return p;
}

// blur_k: fp32 [n_out][3], the 1-D weights of each output; k[1] == 0 means no blur, and that
// block takes k_augment_apply's per-pixel path (the branch is uniform over the block).
template <int ORDER>
__global__ void __launch_bounds__(kBlurTW * kBlurTH)
    k_augment_blur(const uint8_t* __restrict__ img, const dfu_aug_params* __restrict__ params,
                   const int32_t* __restrict__ view_src, const float* __restrict__ blur_k,
                   int n_images, const int32_t* __restrict__ means, int H, int W, int tiles_x,
                   float m0, float m1, float m2, float s0, float s1, float s2,
                   float* __restrict__ out) {
  __shared__ uint32_t tile[kBlurLH * kBlurLW];
  const dfu_aug_params P = params[blockIdx.y];
  const int src = view_image(view_src, blockIdx.y, n_images);
  const uint8_t* im = img + (int64_t)(src < 0 ? 0 : src) * H * W * 3;
  const int n = H * W;
  const int mean = contrast_slot(P) >= 0 ? (int)((2 * (int64_t)means[blockIdx.y] + n) / (2 * (int64_t)n)) : 0;
  const float* bk = blur_k + 3 * (int64_t)blockIdx.y;
  const float k0 = bk[0], k1 = bk[1], k2 = bk[2];
  const int x0 = (int)(blockIdx.x % tiles_x) * kBlurTW, y0 = (int)(blockIdx.x / tiles_x) * kBlurTH;
  const int tx = threadIdx.x % kBlurTW, ty = threadIdx.x / kBlurTW;
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < W && y < H;
  Px p = {{0, 0, 0}};
  if (k1 == 0.f) {
    if (inside) p = augmented<ORDER>(im, P, src, W, H, mean, x, y);
  } else {
    for (int i = threadIdx.x; i < kBlurLH * kBlurLW; i += kBlurTW * kBlurTH) {
      int hx = x0 - 1 + i % kBlurLW, hy = y0 - 1 + i / kBlurLW;
      uint32_t v = 0;
      if (hx <= W && hy <= H) {  // past that no output of this tile reads it
        hx = hx < 0 ? 1 : (hx == W ? W - 2 : hx);
        hy = hy < 0 ? 1 : (hy == H ? H - 2 : hy);
        const Px q = augmented<ORDER>(im, P, src, W, H, mean, hx, hy);
        v = (uint32_t)q.c[0] | (uint32_t)q.c[1] << 8 | (uint32_t)q.c[2] << 16;
      }
      tile[i] = v;
    }
    __syncthreads();
    if (inside) {
      // torchvision's 2-D kernel: fp32(k[j] * k[i]); the nine taps row-major, sequential adds
      const float kk[3] = {k0, k1, k2};
      float acc[3] = {0.f, 0.f, 0.f};
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
          const float w = kk[j] * kk[i];
          const uint32_t v = tile[(ty + j) * kBlurLW + tx + i];
          acc[0] = acc[0] + w * (float)(v & 255u);
          acc[1] = acc[1] + w * (float)(v >> 8 & 255u);
          acc[2] = acc[2] + w * (float)(v >> 16 & 255u);
        }
      for (int c = 0; c < 3; ++c) p.c[c] = (int)rintf(acc[c]);  // torch.round: half to even
    }
  }
  if (inside) {
    float* o = out + (int64_t)blockIdx.y * 3 * n;
    const int i = y * W + x;
    o[i] = ((float)p.c[0] / 255.f - m0) / s0;
    o[n + i] = ((float)p.c[1] / 255.f - m1) / s1;
    o[2 * n + i] = ((float)p.c[2] / 255.f - m2) / s2;
  }
}

template <int ORDER>
int launch_blur(const uint8_t* img, const dfu_aug_params* params, const int32_t* view_src,
                const float* blur_k, int n_images, int n_out, int H, int W, const float* mean3,
                const float* std3, int32_t* contrast_means, float* out, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(contrast_means, 0, sizeof(int32_t) * n_out, stream);
  DFU_CHECK_ARG(e == hipSuccess, "augment: memset: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_augment_stats<ORDER>, dim3(kStatBlocks, n_out), dim3(256), 0, stream, img,
                     params, view_src, n_images, H, W, contrast_means);
  DFU_LAUNCH_CHECK();
  const int tiles_x = (W + kBlurTW - 1) / kBlurTW, tiles_y = (H + kBlurTH - 1) / kBlurTH;
  hipLaunchKernelGGL(k_augment_blur<ORDER>, dim3(tiles_x * tiles_y, n_out),
                     dim3(kBlurTW * kBlurTH), 0, stream, img, params, view_src, blur_k, n_images,
                     contrast_means, H, W, tiles_x, mean3[0], mean3[1], mean3[2], std3[0],
                     std3[1], std3[2], out);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}

}  // namespace

// PIL Resample.c precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter (support 1):
// kernel width of an in_size -> out_size pass.
extern "C" int dfu_resize_ksize(int32_t in_size, int32_t out_size) {
  if (in_size <= 0 || out_size <= 0) return -1;
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(1.0 * filterscale) * 2 + 1;
}

extern "C" int dfu_resize_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds,
                                 int32_t* kk) {
  DFU_CHECK_ARG(in_size > 0 && out_size > 0 && bounds && kk, "dfu_resize_coeffs: bad args");
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = dfu_resize_ksize(in_size, out_size);
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0) t = -t;
      w[x] = t < 1.0 ? 1.0 - t : 0.0;
      ww += w[x];
    }
    for (int x = 0; x < ksize; ++x) {
      double v = x < xmax ? (ww != 0.0 ? w[x] / ww : w[x]) : 0.0;
      kk[(int64_t)xx * ksize + x] =
          (int32_t)(v < 0 ? -0.5 + v * (1 << kPrec) : 0.5 + v * (1 << kPrec));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return DFU_OK;
}

extern "C" int dfu_resize_batch(const uint8_t* src, const dfu_resize_desc* descs,
                                const int32_t* coefs, int32_t n, int32_t out_w, int32_t out_h,
                                uint8_t* tmp, uint8_t* dst, void* stream) {
  DFU_CHECK_ARG(src && descs && coefs && tmp && dst && n > 0 && out_w > 0 && out_h > 0,
                "dfu_resize_batch: bad args");
  hipLaunchKernelGGL(k_resize_h, dim3(96, n), dim3(TPB), 0, (hipStream_t)stream, src, descs,
                     coefs, out_w, tmp);
  DFU_LAUNCH_CHECK();
  const int gx = (out_w * out_h + TPB - 1) / TPB;
  hipLaunchKernelGGL(k_resize_v, dim3(gx < 64 ? gx : 64, n), dim3(TPB), 0, (hipStream_t)stream,
                     tmp, descs, coefs, out_w, out_h, dst);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}

extern "C" int dfu_letterbox_batch(const uint8_t* src, const dfu_resize_desc* descs,
                                   const int32_t* boxes, const int32_t* coefs, int32_t n,
                                   int32_t T, uint8_t* tmp, uint8_t* dst, void* stream) {
  DFU_CHECK_ARG(src && descs && boxes && coefs && tmp && dst, "dfu_letterbox_batch: null pointer");
  DFU_CHECK_ARG(n > 0 && n <= 65535 && T > 0 && (int64_t)T * T * 3 < (1ll << 31),
                "dfu_letterbox_batch: n %d, T %d", n, T);
  hipLaunchKernelGGL(k_letterbox_h, dim3(96, n), dim3(TPB), 0, (hipStream_t)stream, src, descs,
                     boxes, coefs, tmp);
  DFU_LAUNCH_CHECK();
  const int gx = (T * T + TPB - 1) / TPB;
  hipLaunchKernelGGL(k_letterbox_v, dim3(gx < 64 ? gx : 64, n), dim3(TPB), 0,
                     (hipStream_t)stream, tmp, descs, boxes, coefs, T, dst);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}

extern "C" int dfu_augment_normalize(const uint8_t* img, const dfu_aug_params* params, int32_t n,
                                     int32_t H, int32_t W, const float* mean3, const float* std3,
                                     int32_t* contrast_means, float* out, void* stream) {
  DFU_CHECK_ARG(img && params && mean3 && std3 && contrast_means && out && n > 0 && H > 0 &&
                    W > 0 && (int64_t)H * W * 255 < (1ll << 31),
                "dfu_augment_normalize: bad args");
  return launch_augment<DFU_AUG_ORDER_FLIP_ROTATE>(img, params, nullptr, n, n, H, W, mean3, std3,
                                                   contrast_means, out, (hipStream_t)stream);
}

extern "C" int dfu_augment_views(const uint8_t* img, int32_t n_images,
                                 const dfu_aug_params* params, const int32_t* view_src,
                                 int32_t n_views, int32_t order, int32_t H, int32_t W,
                                 const float* mean3, const float* std3, int32_t* contrast_means,
                                 float* out, void* stream) {
  DFU_CHECK_ARG(img && params && view_src && mean3 && std3 && contrast_means && out &&
                    n_images > 0 && n_views > 0 && n_views <= 65535 && H > 0 && W > 0 &&
                    (int64_t)H * W * 255 < (1ll << 31),
                "dfu_augment_views: bad args");
  DFU_CHECK_ARG(order == DFU_AUG_ORDER_FLIP_ROTATE || order == DFU_AUG_ORDER_ROTATE_FLIP,
                "dfu_augment_views: order %d", order);
  if (order == DFU_AUG_ORDER_ROTATE_FLIP)
    return launch_augment<DFU_AUG_ORDER_ROTATE_FLIP>(img, params, view_src, n_images, n_views, H,
                                                     W, mean3, std3, contrast_means, out,
                                                     (hipStream_t)stream);
  return launch_augment<DFU_AUG_ORDER_FLIP_ROTATE>(img, params, view_src, n_images, n_views, H, W,
                                                   mean3, std3, contrast_means, out,
                                                   (hipStream_t)stream);
}

extern "C" int dfu_augment_blur(const uint8_t* img, int32_t n_images, const dfu_aug_params* params,
                                const int32_t* view_src, const float* blur_k, int32_t n_views,
                                int32_t order, int32_t H, int32_t W, const float* mean3,
                                const float* std3, int32_t* contrast_means, float* out,
                                void* stream) {
  DFU_CHECK_ARG(img && params && blur_k && mean3 && std3 && contrast_means && out &&
                    n_images > 0 && n_views > 0 && n_views <= 65535 && H >= 2 && W >= 2 &&
                    (int64_t)H * W * 255 < (1ll << 31),
                "dfu_augment_blur: bad args");
  DFU_CHECK_ARG(order == DFU_AUG_ORDER_FLIP_ROTATE || order == DFU_AUG_ORDER_ROTATE_FLIP,
                "dfu_augment_blur: order %d", order);
  if (order == DFU_AUG_ORDER_ROTATE_FLIP)
    return launch_blur<DFU_AUG_ORDER_ROTATE_FLIP>(img, params, view_src, blur_k, n_images,
                                                  n_views, H, W, mean3, std3, contrast_means, out,
                                                  (hipStream_t)stream);
  return launch_blur<DFU_AUG_ORDER_FLIP_ROTATE>(img, params, view_src, blur_k, n_images, n_views,
                                                H, W, mean3, std3, contrast_means, out,
                                                (hipStream_t)stream);
}
