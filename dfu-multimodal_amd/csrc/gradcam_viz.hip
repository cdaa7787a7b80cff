// The pictures of the Grad-CAM visualisation pass (notebooks/grad_cam_visualization.py:432-462,
// 485-487): per sample the min-max scaled input as a uint8 image, the map resampled to the
// image's size and coloured through a 256-entry table, and the blend of the two.  The script
// does this per sample on the host with numpy and OpenCV; here a whole batch takes
//   dfu_image_minmax   per-image fp32 min and max of the normalised input
//   dfu_cam_overlay    the three uint8 [B][H][W][3] pictures in one pass
// The pixel arithmetic is defined in include/dfu_hip.h (restated from OpenCV's documented
// behaviour, not checked against OpenCV) and is pinned bit for bit by tests/gradcam_viz_ref.py.
#include "common.h"

#pragma clang fp contract(off)  // every product and sum rounds to fp32 on its own, as numpy's

namespace {

constexpr int TPB = 256;
constexpr int MINMAX_PER_BLOCK = TPB * 16;  // elements of one image that one block reduces

__global__ void k_minmax_init(float* __restrict__ minmax, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 2 * B) minmax[i] = (i & 1) ? -__builtin_inff() : __builtin_inff();
}

// min / max of fp32 values by integer atomics on their bit patterns: exact, and no arrival order
// changes the result.  Floats with a clear sign bit order like signed integers and lie above
// every float with the sign bit set; floats with the sign bit set order inversely as unsigned
// integers and lie above (as unsigned) every float with a clear sign bit.  So a value with a
// clear sign bit lowers the minimum by a signed min and raises the maximum by a signed max, and
// a value with the sign bit set lowers the minimum by an unsigned max and raises the maximum by
// an unsigned min; starting from (+inf, -inf) either form leaves an entry it does not improve.
DFU_DEV void atomic_min_f32(float* addr, float v) {
  const uint32_t u = __float_as_uint(v);
  if (u >> 31)
    atomicMax((unsigned int*)addr, u);
  else
    atomicMin((int*)addr, (int)u);
}
DFU_DEV void atomic_max_f32(float* addr, float v) {
  const uint32_t u = __float_as_uint(v);
  if (u >> 31)
    atomicMin((unsigned int*)addr, u);
  else
    atomicMax((int*)addr, (int)u);
}

// Block (g, b) reduces elements [g * MINMAX_PER_BLOCK, +MINMAX_PER_BLOCK) of image b (a
// 3 x 224 x 224 image is 37 blocks) by wave shuffles and LDS, and its first thread folds the
// block's pair into minmax[b] with the two atomics above.
__global__ void __launch_bounds__(TPB) k_image_minmax(const float* __restrict__ x, int n,
                                                      float* __restrict__ minmax) {
  __shared__ float smin[TPB / 64], smax[TPB / 64];
  const int t = threadIdx.x, b = blockIdx.y;
  const float* xb = x + (int64_t)b * n;
  const int lo = blockIdx.x * MINMAX_PER_BLOCK;
  const int hi = min(n - lo, MINMAX_PER_BLOCK) + lo;  // lo < n by the grid's size
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = lo + t; i < hi; i += TPB) {
    const float v = xb[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if ((t & 63) == 0) {
    smin[t >> 6] = mn;
    smax[t >> 6] = mx;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < TPB / 64; ++w) {
      mn = fminf(mn, smin[w]);
      mx = fmaxf(mx, smax[w]);
    }
    atomic_min_f32(minmax + 2 * b, mn);
    atomic_max_f32(minmax + 2 * b + 1, mx);
  }
}

struct OverlayArgs {
  const float* x;
  const float* minmax;
  const float* cam;
  const int32_t *xi0, *xi1, *yi0, *yi1;
  const float *xw, *yw;
  const uint8_t* lut;
  uint8_t *image, *heatmap, *overlay;
  int B, H, W, h, w;
  FastDiv div_hw, div_w;
  float alpha;
  int vec;  // all three outputs are 16-byte aligned: whole chunks go out as one 16-byte store
};

DFU_DEV uint32_t trunc_u8(float v) { return (uint32_t)(int)v & 255u; }

// The 16 bytes of a chunk that starts `off` bytes into the 20-byte window w[0..4].
DFU_DEV u32x4 window16(const uint32_t* w, uint32_t off) {
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], off);
  return r;
}

DFU_DEV void store_chunk(uint8_t* out, int64_t g0, int64_t total, const u32x4 v, int vec) {
  if (vec && g0 + 16 <= total) {
    *(u32x4*)(out + g0) = v;
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)  // the ragged tail, or an unaligned output
    if (g0 + i < total) out[g0 + i] = (uint8_t)(v[i / 4] >> (8 * (i % 4)));
}

// Each of the three outputs is one stream of B * H * W * 3 bytes, cut into 16-byte chunks; thread
// k owns chunk k of all three, so a wave's store is 1 KiB of consecutive bytes.  A chunk begins
// at byte 16 k = 3 p + off of pixel p (off = 0, 1 or 2) and touches the six pixels p .. p + 5:
// the thread computes those six (the first and the last are shared with its neighbours, which
// recompute them), packs their 18 bytes into a window of words and shifts the window by off.
__global__ void __launch_bounds__(TPB) k_cam_overlay(const OverlayArgs a) {
  const int64_t total = (int64_t)a.B * a.H * a.W * 3;
  const int64_t g0 = 16 * (blockIdx.x * (int64_t)TPB + threadIdx.x);
  if (g0 >= total) return;
  const uint32_t npix = (uint32_t)(total / 3), HW = (uint32_t)(a.H * a.W);
  const uint32_t p0 = (uint32_t)(g0 / 3), off = (uint32_t)(g0 - 3 * (int64_t)p0);
  const float beta = 1.0f - a.alpha;
  uint32_t wi[5] = {0, 0, 0, 0, 0}, wh[5] = {0, 0, 0, 0, 0}, wo[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const uint32_t p = p0 + j;
    if (p >= npix) break;  // past the last pixel: bytes past `total`, never stored
    const uint32_t b = fdiv(p, a.div_hw), r = p - b * HW;
    const uint32_t Y = fdiv(r, a.div_w), X = r - Y * (uint32_t)a.W;
    // the map, resampled: horizontal pass on the two source rows, then the vertical one
    const int x0 = min(max(a.xi0[X], 0), a.w - 1), x1 = min(max(a.xi1[X], 0), a.w - 1);
    const int y0 = min(max(a.yi0[Y], 0), a.h - 1), y1 = min(max(a.yi1[Y], 0), a.h - 1);
    const float wx = a.xw[X], wy = a.yw[Y];
    const float* cb = a.cam + (int64_t)b * a.h * a.w;
    const float ux = 1.0f - wx, uy = 1.0f - wy;
    const float t0 = cb[y0 * a.w + x0] * ux + cb[y0 * a.w + x1] * wx;
    const float t1 = cb[y1 * a.w + x0] * ux + cb[y1 * a.w + x1] * wx;
    const float v = t0 * uy + t1 * wy;
    const uint8_t* col = a.lut + 3 * trunc_u8(v * 255.0f);
    const float mn = a.minmax[2 * b], mx = a.minmax[2 * b + 1];
    const float range = mx - mn;
    const float* xp = a.x + (int64_t)b * 3 * HW + r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t img = mx == mn ? 0u : trunc_u8(((xp[(int64_t)c * HW] - mn) / range) * 255.0f);
      const uint32_t heat = col[c];
      const float o = rintf((float)img * beta + (float)heat * a.alpha);
      const uint32_t ov = (uint32_t)fminf(fmaxf(o, 0.0f), 255.0f);
      const int q = 3 * j + c;  // the byte's place in the window
      wi[q / 4] |= img << (8 * (q % 4));
      wh[q / 4] |= heat << (8 * (q % 4));
      wo[q / 4] |= ov << (8 * (q % 4));
    }
  }
  store_chunk(a.image, g0, total, window16(wi, off), a.vec);
  store_chunk(a.heatmap, g0, total, window16(wh, off), a.vec);
  store_chunk(a.overlay, g0, total, window16(wo, off), a.vec);
}

}  // namespace

extern "C" int dfu_image_minmax(const float* x, int32_t B, int32_t n, float* minmax,
                                void* stream) {
  DFU_CHECK_ARG(x && minmax, "dfu_image_minmax: null pointer");
  DFU_CHECK_ARG(B > 0 && B <= 65535 && n > 0, "dfu_image_minmax: B = %d, n = %d", B, n);
  hipLaunchKernelGGL(k_minmax_init, dim3((2 * B + TPB - 1) / TPB), dim3(TPB), 0,
                     (hipStream_t)stream, minmax, B);
  DFU_LAUNCH_CHECK();
  const dim3 grid((n + MINMAX_PER_BLOCK - 1) / MINMAX_PER_BLOCK, B);
  hipLaunchKernelGGL(k_image_minmax, grid, dim3(TPB), 0, (hipStream_t)stream, x, n, minmax);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}

extern "C" int dfu_cam_overlay(const float* x, const float* minmax, const float* cam, int32_t B,
                               int32_t H, int32_t W, int32_t h, int32_t w, const int32_t* xi0,
                               const int32_t* xi1, const float* xw, const int32_t* yi0,
                               const int32_t* yi1, const float* yw, const uint8_t* lut,
                               float alpha, uint8_t* image, uint8_t* heatmap, uint8_t* overlay,
                               void* stream) {
  DFU_CHECK_ARG(x && minmax && cam && lut, "dfu_cam_overlay: null input");
  DFU_CHECK_ARG(xi0 && xi1 && xw && yi0 && yi1 && yw, "dfu_cam_overlay: null tap table");
  DFU_CHECK_ARG(image && heatmap && overlay, "dfu_cam_overlay: null output");
  DFU_CHECK_ARG(B > 0 && H > 0 && W > 0 && h > 0 && w > 0, "dfu_cam_overlay: bad shape");
  DFU_CHECK_ARG((int64_t)B * H * W * 3 < (1ll << 31) && (int64_t)B * h * w < (1ll << 31),
                "dfu_cam_overlay: B * H * W * 3 and B * h * w must stay below 2^31");
  OverlayArgs a;
  a.x = x, a.minmax = minmax, a.cam = cam;
  a.xi0 = xi0, a.xi1 = xi1, a.xw = xw, a.yi0 = yi0, a.yi1 = yi1, a.yw = yw;
  a.lut = lut;
  a.image = image, a.heatmap = heatmap, a.overlay = overlay;
  a.B = B, a.H = H, a.W = W, a.h = h, a.w = w;
  a.div_hw = make_fastdiv((uint32_t)(H * W));
  a.div_w = make_fastdiv((uint32_t)W);
  a.alpha = alpha;
  a.vec = (((uintptr_t)image | (uintptr_t)heatmap | (uintptr_t)overlay) & 15) == 0;
  const int64_t chunks = ((int64_t)B * H * W * 3 + 15) / 16;
  hipLaunchKernelGGL(k_cam_overlay, dim3((unsigned)((chunks + TPB - 1) / TPB)), dim3(TPB), 0,
                     (hipStream_t)stream, a);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}
