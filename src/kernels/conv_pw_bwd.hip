// One-pass backward of the expanding 1x1 convolution of a bottleneck (Cin = 64 -> Cout = 256) on gfx950:
// data gradient and weight gradient from a single read of the output gradient, optionally with the
// residual-tail BatchNorm's backward apply as the prologue.
//
//   g  = APPLY ? round_T(A * (bit ? dy : 0) + B * x3 + Cc) : dY        [M][256]
//   dX = g . W                                                          [M][64]
//   dW = g^T . X                                                        [256][64]
//
// With APPLY, g is the gradient bn_bwd_apply_kernel<T, kReluFromMask, false> (bn_nhwc.hip) would have
// stored, formed in registers with the same expression and the same rounding, so it is never written:
// the separate kernels stream it three times (one write, two reads of 2 * M * 256 bytes).
//
//   * persistent workgroups of 512 threads; workgroup b walks the 64-pixel chunks [b * cpb, (b + 1) * cpb),
//     cpb = ceil(chunks / blocks), in order (the pixel -> workgroup map depends on (M, blocks) alone, no atomics, no
//     communication between workgroups);
//   * operands are register-staged because they are transformed on the way: each thread keeps one
//     8-channel group of the 256 (its A / B / Cc live in registers) and loads 4 rows of dy, x3 and the
//     mask bytes per chunk, plus one 16-byte piece of X; two register sets, so a chunk and a half are in
//     flight while the current one is in the MFMAs;
//   * g goes to four swizzled [64 pixel][64 channel] LDS sub-tiles and X to a fifth (the layout and
//     swizzle of conv_wgrad.hip); dX reads g rows as they lie (B fragments) against W^T from LDS, dW reads
//     both images with the transposing ds_read_b64_tr_b16; both images and the dX row image are
//     double-buffered, one barrier per chunk;
//   * dW accumulates in registers over the workgroup's whole life (8 waves x 8 16x16 tiles) and is
//     written once as an fp32 slab row [blocks][256 * 64]; a workgroup without pixels writes zeros.  The
//     caller sums the slab with the one-launch slab reduce.
//
// Rows past M contribute zeros and are not stored.
#include <stdexcept>

#include "common.h"
#include "mfma.h"

namespace mxamd {

namespace {

typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

constexpr int kCin = 64, kCout = 256, kBM = 64;
constexpr int kSub = 64 * 64 * 2;              // one [64][64] sub-tile, bytes
constexpr int kGImg = 4 * kSub;                // g image: sub-tile per 64 output channels
constexpr int kXImg = kSub;
constexpr int kDxPitch = kCin * 2 + 16;        // dX row image, conflict-free 8-byte writes
constexpr int kDxImg = kBM * kDxPitch;
constexpr int kBuf = kGImg + kXImg + kDxImg;   // one stage
constexpr int kWPitch = kCout * 2 + 16;        // W^T image [64][256], rows 16 bytes apart in the bank row
constexpr int kWImg = kCin * kWPitch;
constexpr int kSmem = 2 * kBuf + kWImg;
static_assert(kSmem <= 160 * 1024, "LDS of one CU");

// conv_wgrad.hip's sub-tile swizzle: the 16-byte chunk of row r is XORed with this
__device__ __forceinline__ int swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }

// 8 consecutive rows (pixels) of one column (channel) as an MFMA fragment: two transposing reads over rows
// [8g+q] and [8g+4+q] (conv_wgrad.hip's lds_tr pattern)
__device__ __forceinline__ v8s tr_frag(const char* tile, int off) {
  typedef __attribute__((address_space(3))) char lds_char;
  lds_char* base = (lds_char*)(tile);
  v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(base + off));
  v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(base + off + 512));
  return v8s{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ u32x4 load_nt(const void* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

template <bool APPLY>
struct Stage {
  u32x4 dy[4];
  u32x4 x3[APPLY ? 4 : 1];
  uint32_t mb[APPLY ? 4 : 1];
  u32x4 xin;
};

template <typename T, bool APPLY>
__global__ void __launch_bounds__(512) conv_pw_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x3,
                                                          const uint8_t* __restrict__ mask,
                                                          const float* __restrict__ A, const float* __restrict__ B,
                                                          const float* __restrict__ Cc, const T* __restrict__ X,
                                                          const T* __restrict__ wt, T* __restrict__ dX,
                                                          float* __restrict__ slab, int M) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int nchunks = (M + kBM - 1) / kBM;
  const int bid = blockIdx.x, grid = gridDim.x;
  // One contiguous pixel range per workgroup, walked in order, and the MFMA sequence per chunk of
  // conv_wgrad.hip: with `blocks` = that file's split count this is its plan (ranges of
  // 64 * ceil(ceil(M / 64) / blocks) pixels), so the slab, and after the same reduce dW, equal the in-tree
  // weight gradient's bit for bit (one workgroup per CU is the ring kernels' plan for this weight).
  const int cpb = (nchunks + grid - 1) / grid;
  const int c0 = bid * cpb;
  const int n = min(max(nchunks - c0, 0), cpb);   // chunks of this workgroup

  // ---- staging geometry: 8-channel group cg of rows r0, r0+16, r0+32, r0+48; X piece (xr, xc)
  const int cg = tid & 31, r0 = tid >> 5;
  const int xr = tid >> 3, xc = tid & 7;
  float ka[8], kb[8], kc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    ka[q] = APPLY ? A[cg * 8 + q] : 0.f;
    kb[q] = APPLY ? B[cg * 8 + q] : 0.f;
    kc[q] = APPLY ? Cc[cg * 8 + q] : 0.f;
  }

  // ---- W^T [64 c][256 k] into its LDS image (read by the dX MFMAs of every chunk)
  char* wimg = smem + 2 * kBuf;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + i * 512;   // 16-byte piece: row e / 32, piece e % 32
    *reinterpret_cast<u32x4*>(wimg + (e >> 5) * kWPitch + (e & 31) * 16) =
        *reinterpret_cast<const u32x4*>(wt + static_cast<int64_t>(e) * 8);
  }

  // rows past M load the last row (no divergent loads) and are zeroed when the stage is committed
  auto load = [&](Stage<APPLY>& s, int chunk) {
    const int p0 = chunk * kBM;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = min(p0 + r0 + 16 * i, M - 1);
      const int64_t e = static_cast<int64_t>(p) * kCout + cg * 8;
      s.dy[i] = load_nt(dy + e);
      if (APPLY) {
        s.x3[i] = load_nt(x3 + e);
        s.mb[i] = mask[e >> 3];
      }
    }
    s.xin = *reinterpret_cast<const u32x4*>(X + static_cast<int64_t>(min(p0 + xr, M - 1)) * kCin + xc * 8);
  };

  // transform and write the stage's chunk to the LDS images of `buf`
  auto commit = [&](const Stage<APPLY>& s, int chunk, char* buf) {
    const int p0 = chunk * kBM;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + 16 * i;
      Vec8<T> g;
      g.raw = __builtin_bit_cast(uint4, s.dy[i]);
      if (APPLY) {
        Vec8<T> d = g, xv;
        xv.raw = __builtin_bit_cast(uint4, s.x3[i]);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma clang fp contract(off)
          // bn_bwd_apply_kernel's ka * d + kb * x + kc with the roundings its fixed-channel path compiles to
          // (every C that divides 2048 takes that path): round(ka * d), one fused kb * x + that, then + kc;
          // spelled out so that no other contraction can be chosen here, and rounded to T by the same conversion
          const float dd = ((s.mb[i] >> q) & 1u) ? d.get(q) : 0.f;
          const float t = ka[q] * dd;
          g.set(q, fmaf(kb[q], xv.get(q), t) + kc[q]);
        }
      }
      if (p0 + r >= M) g.raw = make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4*>(buf + (cg >> 3) * kSub + r * 128 + (((cg & 7) ^ swz(r)) << 4)) = g.raw;
    }
    u32x4 xv = s.xin;
    if (p0 + xr >= M) xv = u32x4{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(buf + kGImg + xr * 128 + ((xc ^ swz(xr)) << 4)) = xv;
  };

  // ---- MFMA geometry
  // dX^T tile of wave w: pixel fragment w >> 1, channel fragments 2 (w & 1) + {0, 1}; A = W^T rows (c), B = g
  // rows (pixel), so a lane ends with 4 consecutive c of one pixel
  const int pf = wid >> 1, ch = wid & 1;
  const int grow = pf * 16 + (lane & 15);                       // g image row of this lane's B fragment
  const int gswz = swz(grow);
  const int wrow0 = (ch * 32 + (lane & 15)) * kWPitch + (lane >> 4) * 16;
  // dW tile of wave w: g sub-tile w >> 1 (64 k), its fragments 2 (w & 1) + {0, 1}, all 4 X fragments
  const int fg = lane >> 4, fq = (lane >> 2) & 3, fp = lane & 3;
  const int frow = 8 * fg + fq;
  auto frag_off = [&](int f) { return frow * 128 + ((((2 * f) + (fp >> 1)) ^ swz(frow)) << 4) + ((fp & 1) << 3); };
  int foff[4], goff[2];   // X fragments 0..3; this wave's two g fragments (statically indexed: registers)
#pragma unroll
  for (int f = 0; f < 4; ++f) foff[f] = frag_off(f);
#pragma unroll
  for (int j = 0; j < 2; ++j) goff[j] = frag_off(2 * ch + j);

  f4_t accw[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) accw[i][j] = f4_t{0.f, 0.f, 0.f, 0.f};

  // the dX rows of the chunk whose image lies in `buf`: one 16-byte piece per thread
  auto store_dx = [&](int chunk, const char* buf) {
    const int p = chunk * kBM + xr;
    if (p < M)
      *reinterpret_cast<uint4*>(dX + static_cast<int64_t>(p) * kCin + xc * 8) =
          *reinterpret_cast<const uint4*>(buf + kGImg + kXImg + xr * kDxPitch + xc * 16);
  };

  auto mfmas = [&](char* buf) {
    // dX^T = W^T . g^T over the 256 output channels
    f4_t accx[2] = {f4_t{0.f, 0.f, 0.f, 0.f}, f4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int c8 = (s & 1) * 4 + (lane >> 4);
      const u32x4 gb = *reinterpret_cast<const u32x4*>(buf + (s >> 1) * kSub + grow * 128 + ((c8 ^ gswz) << 4));
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const u32x4 wa = *reinterpret_cast<const u32x4*>(wimg + wrow0 + f * 16 * kWPitch + s * 64);
        accx[f] = mfma::Op<T>::run(wa, gb, accx[f]);
      }
    }
    // dW += X^T . g over the chunk's 64 pixels (rows = c, columns = k)
    const char* gsub = buf + pf * kSub;
    const char* ximg = buf + kGImg;
#pragma unroll
    for (int kk = 0; kk < 64; kk += 32) {
      v8s a[4], b[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = tr_frag(gsub, kk * 128 + goff[j]);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = tr_frag(ximg, kk * 128 + foff[i]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) accw[i][j] = mfma::Op<T>::run(a[i], b[j], accw[i][j]);
    }
    // dX row image: lane holds c = 32 ch + 16 f + 4 (lane >> 4) + {0..3} of pixel 16 pf + (lane & 15)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int c = ch * 32 + f * 16 + (lane >> 4) * 4;
      *reinterpret_cast<uint2*>(buf + kGImg + kXImg + grow * kDxPitch + c * 2) =
          mfma::Op<T>::pack4(accx[f][0], accx[f][1], accx[f][2], accx[f][3]);
    }
  };

  // chunk j of this workgroup: stage -> images of buffer j & 1, refill the stage with chunk j + 2, one
  // barrier, then the previous chunk's dX rows (their image is complete behind the barrier) and the MFMAs.
  // Buffer j & 1 is written again in step j + 2, behind barrier j + 1, which every wave reaches only after
  // its reads of step j.
  auto step = [&](Stage<APPLY>& s, int j, int b) {
    char* buf = smem + b * kBuf;
    commit(s, c0 + j, buf);
    if (j + 2 < n) load(s, c0 + j + 2);
    __syncthreads();
    if (j > 0) store_dx(c0 + j - 1, smem + (b ^ 1) * kBuf);
    mfmas(buf);
  };

  Stage<APPLY> sa, sb;
  if (n > 0) load(sa, c0);
  if (n > 1) load(sb, c0 + 1);
  for (int j = 0; j < n; j += 2) {
    step(sa, j, 0);
    if (j + 1 < n) step(sb, j + 1, 1);
  }
  if (n > 0) {
    __syncthreads();
    store_dx(c0 + n - 1, smem + ((n - 1) & 1) * kBuf);
  }

  // ---- slab row of this workgroup: [k][c], lane holds c = 16 i + 4 (lane >> 4) + {0..3} of one k
  float* out = slab + static_cast<int64_t>(bid) * (kCout * kCin);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = pf * 64 + (2 * ch + j) * 16 + (lane & 15);
      *reinterpret_cast<f4_t*>(out + k * kCin + i * 16 + (lane >> 4) * 4) = accw[i][j];
    }
}

template <typename T, bool APPLY>
void launch_pw_bwd(const void* dy, const void* x3, const uint8_t* mask, const float* A, const float* B,
                   const float* Cc, const void* X, const void* wt, void* dX, float* slab, int M, int blocks,
                   hipStream_t s) {
  static bool set = false;
  if (!set) {
    MXAMD_HOST_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_pw_bwd_kernel<T, APPLY>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, kSmem) == hipSuccess,
                     "conv_pw_bwd: the kernel needs 134 KB of LDS");
    set = true;
  }
  hipLaunchKernelGGL((conv_pw_bwd_kernel<T, APPLY>), dim3(blocks), dim3(512), kSmem, s, static_cast<const T*>(dy),
                     static_cast<const T*>(x3), mask, A, B, Cc, static_cast<const T*>(X), static_cast<const T*>(wt),
                     static_cast<T*>(dX), slab, M);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int conv_pw_bwd_ok(int cin, int cout) { return cin == kCin && cout == kCout ? 1 : 0; }

// dy [M][256], X [M][64], wt = W^T [64][256], dX [M][64], slab [blocks][256 * 64] fp32 (every row written).
// x3 != null: dy is the residual tail's incoming gradient and g = A * (mask bit ? dy : 0) + B * x3 + Cc is
// formed on the way (mask: one bit per element, A / B / Cc: 256 floats each).
void conv_pw_bwd(int dtype, const void* dy, const void* x3, const uint8_t* mask, const float* A, const float* B,
                 const float* Cc, const void* X, const void* wt, void* dX, float* slab, int64_t M, int cin, int cout,
                 int blocks, hipStream_t s) {
  MXAMD_HOST_CHECK(conv_pw_bwd_ok(cin, cout), "conv_pw_bwd: built for Cin = 64, Cout = 256 only");
  MXAMD_HOST_CHECK(dtype == kF16 || dtype == kBF16, "conv_pw_bwd: dtype must be f16 or bf16");
  MXAMD_HOST_CHECK(M >= 1 && M * kCout < (1ll << 31), "conv_pw_bwd: pixel count out of range");
  MXAMD_HOST_CHECK(blocks >= 1 && blocks <= 4096, "conv_pw_bwd: workgroup count out of range");
  MXAMD_HOST_CHECK(dy && X && wt && dX && slab && aligned16(dy) && aligned16(X) && aligned16(wt) && aligned16(dX) &&
                       aligned16(slab),
                   "conv_pw_bwd: operands must be non-null and 16-byte aligned");
  const bool apply = x3 != nullptr;
  MXAMD_HOST_CHECK(!apply || (mask && A && B && Cc && aligned16(x3)),
                   "conv_pw_bwd: the BatchNorm prologue needs x3 (16-byte aligned), the mask and A / B / Cc");
  const int m = static_cast<int>(M);
  if (dtype == kF16) {
    if (apply) launch_pw_bwd<__half, true>(dy, x3, mask, A, B, Cc, X, wt, dX, slab, m, blocks, s);
    else launch_pw_bwd<__half, false>(dy, x3, mask, A, B, Cc, X, wt, dX, slab, m, blocks, s);
  } else {
    if (apply) launch_pw_bwd<__hip_bfloat16, true>(dy, x3, mask, A, B, Cc, X, wt, dX, slab, m, blocks, s);
    else launch_pw_bwd<__hip_bfloat16, false>(dy, x3, mask, A, B, Cc, X, wt, dX, slab, m, blocks, s);
  }
}

}  // namespace mxamd
