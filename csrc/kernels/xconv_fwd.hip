// fp32 family, forward pass (xconv.hpp): the conv launcher (halo / whole-image / implicit-GEMM
// tiles, split-K in-launch or in-block, fused training-BN statistics and lazy BN operands), the
// evaluation down-block, and the whole-image halo conv of the 8 / 4-wide evaluation stages in its
// two forms (ximg2_kernel: B fragments from global memory, two patch buffers; ximg_kernel: the
// LDS weight ring).
#include "xhalo.hpp"

namespace xg {
SplitPolicy& split_policy() {
  static SplitPolicy p;
  return p;
}
int& xstage_mode() {
  static int mode = 1;
  return mode;
}
XLast& last_launch() {
  static XLast l{};
  return l;
}
}  // namespace xg

namespace {

// ================================================================ whole-image halo conv
// (The first form: since ximg2_kernel below it runs only for weights without fragment-ordered
// planes — fp32 weights split while staging, PRE false — and as dba_ximg_set(2), the bit-equality
// test's and the kernel bench's A/B.)
// Stride-1 3x3 pad-1 evaluation forward of the small-image stages (W 8 / 4: ResNet stages
// 3-4 on 32x32 inputs; fp16 pair, weights pre-split at the eval fold).  The implicit GEMM
// re-fetches every input element once per tap, and at these shapes its operand fetch — not
// the MFMA — bounds it (eval.layer3 / 4 ran +37 / +43 % faster with the in-loop global loads
// removed, against +5 % without the in-loop barriers: profiles/r4/ximg).  Here a block owns
// IMGS whole images (BM = 128 output pixels) x BN output channels; the reduction runs
// channel-chunk-major (chunk of 32 channels, then its 9 taps): each chunk's zero-padded patch
// (IMGS x (W+2)^2 pixels x 32 channels) is loaded once, split once into the LDS patch, and
// read by all 9 taps at their pixel offsets — (W+2)^2 / W^2 = 1.27x / 1.56x / 2.25x of the
// image bytes (W 16 / 8 / 4) instead of 9x.  The next chunk's patch is loaded into registers while the
// current chunk's 9 k-steps run (8 steps to land).
// 4 waves, 2 blocks per CU, one patch buffer: the next chunk is split + stored after the
// chunk's last barrier (one more barrier per chunk).  (An 8-wave BM-256 form with two patch
// buffers, the next chunk split in the MFMA gaps, was measured slower — one block per CU
// exposes its prologue / epilogue: eval.layer3 254 vs 314 TF, profiles/r4/ximg/README.md.)
// Weights: the two-stage register / LDS ring of xhalo_kernel, one barrier per k-step (global ->
// VGPR -> LDS -> VGPR in every block: ximg2_kernel's first saving).  Epilogue straight from the
// accumulators (a 32-lane row is 32 consecutive output channels: 128-B segments).
// (A fused downsampling shortcut as extra one-tap chunks — each refilling the patch, its loads
// prefetched only two k-steps ahead — measured slower than the shortcut conv + this kernel with a
// residual epilogue: 17 x 1024 images, layer3.0 1534 vs 1467 us, layer4.0 1370 vs 1142 us,
// profiles/r5/down/kbench_ximg_sc.log; the W-16 halo kernel's fused form wins: xhalo_kernel SC.)
// Deterministic; the chunk-major k order makes its bits differ from the tap-major implicit
// GEMM's (both fp32 level: tests hold both to the fp64 oracle).
template <int W, int IMGS, int BN, int WM, int WN, bool PRE>
__global__ __launch_bounds__(256) void ximg_kernel(const XArgs a) {
  constexpr int P = 2, NT = 256;
  constexpr int PW = W + 2, PI = PW * PW, PP = IMGS * PI;   // padded pixels per image / patch
  constexpr int CC = 32, CH = CC / 8, Q4 = CC / 4;          // chunk channels, 16-B chunks, float4 per pixel
  constexpr int PATCH = PP * CH;                            // uint4 per plane
  constexpr int BM = IMGS * W * W;
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NJ = TN / 32;
  static_assert(WM * WN == NT / 64 && MI >= 1 && NJ >= 1 && BM == 128, "tiling");
  constexpr int RPT = NT / 8;                               // weight rows staged per pass
  static_assert(BN % RPT == 0, "weight rows");
  constexpr int RB = BN / RPT, BPL = BN * 4;
  __shared__ __attribute__((aligned(16))) uint4 patch[P * PATCH];
  __shared__ __attribute__((aligned(16))) uint4 bring[2 * P * BPL];

  const int g = blockIdx.y;
  const int tn = blockIdx.x % a.tiles_n, tm = blockIdx.x / a.tiles_n;
  const int img0 = tm * IMGS, n0 = tn * BN;
  const int nv = min(valid_rows(a.nvalid, g, a.N), a.N);
  if (img0 >= nv) return;
  const int slot = a.wsel ? a.wsel[g] : g;
  const int Cs = a.Cs, K = 9 * Cs, NC = Cs / CC, NK = 9 * NC;
  const float* __restrict__ src = a.src + (long long)g * a.src_gstride;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int kq = tid & 7, r0 = tid >> 3;
  const int fr = lane & 31, hf = lane >> 5;

  // ---- patch chunks: chunk cc of images img0 .. img0+IMGS-1, zero padding / invalid images
  constexpr int NE = (PP * Q4 + NT - 1) / NT;
  float4 pv[NE];
  const __amdgpu_buffer_rsrc_t rA = rsrc(src, (long long)a.N * W * W * Cs * 4);
  auto pload = [&](int cc) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + NT * u;
      const int pp = e / Q4, q = e - pp * Q4;
      const int im = pp / PI, rem = pp - im * PI;
      const int h = rem / PW - 1, w = rem % PW - 1, img = img0 + im;
      const bool ok = e < PP * Q4 && img < nv && (unsigned)h < (unsigned)W && (unsigned)w < (unsigned)W;
      pv[u] = bload4(rA, ok ? (((img * W + h) * W + w) * Cs + cc * CC + q * 4) * 4 : kOOB);
    }
  };
  HScale hs;
  auto ppiece = [&](int u, float m) __attribute__((always_inline)) {   // piece u of pv -> the patch
    const int e = tid + NT * u;
    if (e >= PP * Q4) return;
    const int pp = e / Q4, q = e - pp * Q4;
    const int prow = (pp % PI) / PW;   // patch row: the swizzle key
    uint2 sp[P];
    split4h(pv[u].x, pv[u].y, pv[u].z, pv[u].w, m, sp);
    const int o = pp * CH + ((q >> 1) ^ (prow & 3));
#pragma unroll
    for (int p = 0; p < P; ++p) ((uint2*)&patch[p * PATCH + o])[q & 1] = sp[p];
  };

  // ---- weights (pre-split planes, or fp32 split while staging: the same bits): two-stage
  // pipeline, k-step t = chunk t / 9, tap t % 9
  int bn_[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int n = n0 + r0 + RPT * j;
    bn_[j] = n < a.Ncol ? n : -1;
  }
  const uint16_t* Bh = PRE ? a.wp + (long long)slot * a.wp_sstride : nullptr;
  const __amdgpu_buffer_rsrc_t rBh = rsrc(Bh, (long long)a.Ncol * K * 2);
  const __amdgpu_buffer_rsrc_t rBl = rsrc(PRE ? Bh + (a.wp_sstride >> 1) : nullptr, (long long)a.Ncol * K * 2);
  const __amdgpu_buffer_rsrc_t rB = rsrc(a.w + (long long)slot * a.w_sstride, (long long)a.Ncol * K * 4);
  uint4 rb[2][RB];
  auto gq = [&](int t, int st, int j) __attribute__((always_inline)) {
    const bool ok = bn_[j] >= 0 && t < NK;
    const int cc = t / 9, tap = t - cc * 9;
    const int kb = bn_[j] * K + tap * Cs + cc * CC + kq * 4;
    if constexpr (PRE) {
      const uint2 h = bload8(rBh, ok ? kb * 2 : kOOB), l = bload8(rBl, ok ? kb * 2 : kOOB);
      rb[st][j] = make_uint4(h.x, h.y, l.x, l.y);
    } else {
      rb[st][j] = __builtin_bit_cast(uint4, bload4(rB, ok ? kb * 4 : kOOB));
    }
  };
  auto lput_q = [&](int buf, int st, int q) __attribute__((always_inline)) {
    uint2 sp[P];
    if constexpr (PRE) {
      sp[0] = make_uint2(rb[st][q].x, rb[st][q].y);
      sp[1] = make_uint2(rb[st][q].z, rb[st][q].w);
    } else {
      const float4 v = __builtin_bit_cast(float4, rb[st][q]);
      split4h(v.x, v.y, v.z, v.w, hs.mb, sp);
    }
    lds_put<P, false, BN>(bring + buf * P * BPL, BPL, 0, r0 + RPT * q, kq, sp);
  };

  f32x16_t acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // patch pixel and patch row of each A fragment row at tap (0, 0).  LDS image: pixel pp holds
  // 4 16-B chunks, chunk c at c ^ (patch row & 3) — the rows of a 32-lane fragment read (W 8: 4
  // rows of 8 pixels, W 4: 2 images x 4 rows of 4) then hit 16 distinct 16-B bank slots in each
  // ds_read_b128 lane group at every tap (the 32-wide halo conv's (pp >> 2) & 3 left 2-way
  // conflicts here: SQ_LDS_BANK_CONFLICT 8.0e7 per launch, profiles/r4/final2/)
  int apix[MI], arow[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = wm * TM + i * 32 + fr;
    const int im = m / (W * W), rem = m - im * (W * W);
    apix[i] = im * PI + (rem / W) * PW + rem % W;
    arow[i] = rem / W;
  }
  // k-step t from weight buffer buf; fill: the weight ring's next step
  auto mma = [&](int t, int buf, int stn) __attribute__((always_inline)) {
    const int tap = t % 9, ti = tap / 3, tj = tap - ti * 3;
    const int toff = ti * PW + tj;
    const uint4* L = bring + buf * P * BPL;
    sfor<2>([&](auto KK) __attribute__((always_inline)) {
      const int ch = decltype(KK)::value * 2 + hf;
      uint4 af[P][MI], bfr[P][NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int pp = apix[i] + toff;
        const int o = pp * CH + (ch ^ ((arow[i] + ti) & 3));
#pragma unroll
        for (int p = 0; p < P; ++p) af[p][i] = patch[p * PATCH + o];
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = wn * TN + j * 32 + fr;
        const int o = n * 4 + (ch ^ ((n >> 2) & 3));
#pragma unroll
        for (int p = 0; p < P; ++p) bfr[p][j] = L[p * BPL + o];
      }
      mma_half<MI, NJ, P, true, RB, decltype(KK)::value>(af, bfr, acc, [&](int q) __attribute__((always_inline)) {
        lput_q(buf ^ 1, stn, q);
        gq(t + 3, stn, q);   // reload: step t+3 (past NK: zero-filled, never read)
      });
    });
  };
  auto step = [&](int t, int buf, int stn) __attribute__((always_inline)) {
    const int c = t / 9;
    mma(t, buf, stn);
    __syncthreads();
    if (t - 9 * c == 8 && c + 1 < NC) {   // the chunk's last k-step, another follows
#pragma unroll
      for (int u = 0; u < NE; ++u) ppiece(u, hs.ma);   // every read of the old patch is done
      if (c + 2 < NC) pload(c + 2);
      __syncthreads();
    }
  };

  hs.init(amax_read(a.amax_src, a.amax_src_ld, g), amax_read(a.amax_w, a.amax_w_ld, slot));
#pragma unroll
  for (int q = 0; q < RB; ++q) {
    gq(0, 0, q);
    gq(1, 1, q);
  }
  pload(0);
#pragma unroll
  for (int u = 0; u < NE; ++u) ppiece(u, hs.ma);
  if (NC > 1) pload(1);
#pragma unroll
  for (int q = 0; q < RB; ++q) {
    lput_q(0, 0, q);
    gq(2, 0, q);
  }
  __syncthreads();   // patch (chunk 0) + first weight step
  int t = 0;
  for (; t + 1 < NK; t += 2) {
    step(t, 0, 1);
    step(t + 1, 1, 0);
  }
  if (t < NK) step(t, 0, 1);
  hs.finish(acc);

  // ---- epilogue from the accumulators: bias, residual, ReLU, max
  float* out = a.out + (long long)g * a.out_gstride;
  const float* bias = a.bias ? a.bias + (long long)slot * a.b_sstride : nullptr;
  const float* res = a.res ? a.res + (long long)g * a.out_gstride : nullptr;
  float vmax = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = n0 + wn * TN + j * 32 + fr;
    if (n >= a.Ncol) continue;
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
        if (img0 + m / (W * W) >= nv) continue;
        const long long o = (long long)(img0 * W * W + m) * a.Ncol + n;
        float v = acc[i][j][r];
        if (bias) v += bv;
        if (res) v += res[o];
        if (a.relu) v = relu_nan(v);
        vmax = fmaxf(vmax, fabsf(v));
        out[o] = v;
      }
  }
  if (a.amax_out) amax_fold(a.amax_out, a.amax_out_ld, g, vmax);
}

// ================================================================ whole-image halo conv, 2nd form
// ximg_kernel's tiles, patch, k order and epilogue (so every output element sees the same
// MFMA sequence: the same bits), without its two costs that the result does not need
// (profiles/r4/ximg: +13 / +15 % without the in-loop weight loads, +9 % without the
// chunk-boundary refill):
//  * B fragments come straight from global memory: the weights are fragment-ordered once at the
//    fold (xaux.hip xfrag_w_kernel: per (32-column tile, k-step, half-step, plane) one 1-KB
//    block, lane l's 16 B at 16 l), so a fragment is one buffer_load_dwordx4 per lane, two
//    k-steps ahead in a 3-slot register ring — no LDS weight ring, no swizzled ds_write /
//    ds_read of weights, no barrier per k-step.  A wave owns all 128 rows x 32 columns
//    (WM = 1; BN 64: 2 x 2 waves of 64 x 32), so each fragment is loaded by one wave of the block.
//  * Two patch buffers (the LDS the weight ring held): the next chunk's patch registers are
//    split and stored into the other buffer one piece per k-step in the MFMA gaps (the fill
//    hook of mma_half), each piece's reload for the chunk after issued right behind it.  One
//    barrier per chunk.  W 4: 2 x 36.9 KB of dynamic LDS (two blocks per CU: 147 of 160 KB).
// 17 x 1024 images, same box: eval.layer3 321 -> 370, eval.layer4 362 -> 417 TFLOP/s
// (profiles/r7/ximg2/README.md).
template <int W, int IMGS, int BN>
__global__ __launch_bounds__(256) void ximg2_kernel(const XArgs a) {
  constexpr int P = 2, NT = 256;
  constexpr int PW = W + 2, PI = PW * PW, PP = IMGS * PI;   // padded pixels per image / patch
  constexpr int CC = 32, CH = CC / 8, Q4 = CC / 4;          // chunk channels, 16-B chunks, float4 per pixel
  constexpr int PATCH = PP * CH;                            // uint4 per plane
  constexpr int BM = IMGS * W * W;
  constexpr int WN = BN / 32, WM = (NT / 64) / WN, TM = BM / WM, MI = TM / 32;
  static_assert(WM * WN == NT / 64 && MI >= 1 && BM == 128, "tiling");
  extern __shared__ __attribute__((aligned(16))) uint4 ximg2_patch[];   // [2 buffers][P][PATCH]

  const int g = blockIdx.y;
  const int tn = blockIdx.x % a.tiles_n, tm = blockIdx.x / a.tiles_n;
  const int img0 = tm * IMGS, n0 = tn * BN;
  const int nv = min(valid_rows(a.nvalid, g, a.N), a.N);
  if (img0 >= nv) return;
  const int slot = a.wsel ? a.wsel[g] : g;
  const int Cs = a.Cs, NC = Cs / CC, NK = 9 * NC;
  const float* __restrict__ src = a.src + (long long)g * a.src_gstride;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int fr = lane & 31, hf = lane >> 5;

  // ---- patch pieces: piece u of chunk cc (zero padding / invalid images / past the last chunk)
  constexpr int NE = (PP * Q4 + NT - 1) / NT;
  static_assert(NE <= 9, "one patch piece per k-step");
  float4 pv[NE];
  const __amdgpu_buffer_rsrc_t rA = rsrc(src, (long long)a.N * W * W * Cs * 4);
  auto pload1 = [&](int u, int cc) __attribute__((always_inline)) {
    const int e = tid + NT * u;
    const int pp = e / Q4, q = e - pp * Q4;
    const int im = pp / PI, rem = pp - im * PI;
    const int h = rem / PW - 1, w = rem % PW - 1, img = img0 + im;
    const bool ok = e < PP * Q4 && cc < NC && img < nv && (unsigned)h < (unsigned)W && (unsigned)w < (unsigned)W;
    pv[u] = bload4(rA, ok ? (((img * W + h) * W + w) * Cs + cc * CC + q * 4) * 4 : kOOB);
  };
  HScale hs;
  auto ppiece = [&](int u, int buf) __attribute__((always_inline)) {   // piece u of pv -> patch buffer buf
    const int e = tid + NT * u;
    if (NT * (u + 1) > PP * Q4 && e >= PP * Q4) return;   // (only the last piece can be partial)
    const int pp = e / Q4, q = e - pp * Q4;
    const int prow = (pp % PI) / PW;   // patch row: the swizzle key
    uint2 sp[P];
    split4h(pv[u].x, pv[u].y, pv[u].z, pv[u].w, hs.ma, sp);
    const int o = pp * CH + ((q >> 1) ^ (prow & 3));
#pragma unroll
    for (int p = 0; p < P; ++p) ((uint2*)&ximg2_patch[(buf * P + p) * PATCH + o])[q & 1] = sp[p];
  };

  // ---- weights: fragment f = half-step * 2 + plane of k-step t (chunk t / 9, tap t % 9) of
  // this wave's 32 columns, ring slot t % 3
  const __amdgpu_buffer_rsrc_t rF = rsrc(a.wf + (long long)slot * a.wf_sstride, (long long)a.Ncol * 9 * Cs * 4);
  const int wbase = ((n0 >> 5) + wn) * NK * 4096 + lane * 16;
  uint4 wb[3][4];
  auto gw = [&](int t, int s, int f) __attribute__((always_inline)) {
    wb[s][f] = __builtin_bit_cast(uint4, bload4(rF, t < NK ? wbase + t * 4096 + f * 1024 : kOOB));
  };

  f32x16_t acc[MI][1];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;

  // patch pixel and patch row of each A fragment row at tap (0, 0) (ximg_kernel's image)
  int apix[MI], arow[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = wm * TM + i * 32 + fr;
    const int im = m / (W * W), rem = m - im * (W * W);
    apix[i] = im * PI + (rem / W) * PW + rem % W;
    arow[i] = rem / W;
  }

  hs.init(amax_read(a.amax_src, a.amax_src_ld, g), amax_read(a.amax_w, a.amax_w_ld, slot));
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    gw(0, 0, f);
    gw(1, 1, f);
  }
#pragma unroll
  for (int u = 0; u < NE; ++u) pload1(u, 0);
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    ppiece(u, 0);
    pload1(u, 1);
  }
  __syncthreads();   // patch (chunk 0)
  for (int c = 0; c < NC; ++c) {
    const uint4* L = ximg2_patch + (c & 1) * P * PATCH;
    const bool more = c + 1 < NC;
    sfor<9>([&](auto TAP) __attribute__((always_inline)) {
      constexpr int tap = decltype(TAP)::value, ti = tap / 3, tj = tap - ti * 3;
      constexpr int toff = ti * PW + tj, s = tap % 3, s2 = (tap + 2) % 3;
      constexpr int u = tap - (9 - NE);           // the patch piece refilled beside this k-step
      constexpr int NQ = u >= 0 ? 5 : 4;
      const int t = c * 9 + tap;
      // no global load and no MFMA crosses a k-step boundary (VALU / SALU / LDS may): left alone,
      // the scheduler sinks the ring's loads down to their MFMAs, two steps later, and their
      // latency is exposed
      __builtin_amdgcn_sched_barrier(0x786);
      sfor<2>([&](auto KK) __attribute__((always_inline)) {
        constexpr int kk = decltype(KK)::value;
        const int ch = kk * 2 + hf;
        uint4 af[P][MI], bfr[P][1];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const int o = (apix[i] + toff) * CH + (ch ^ ((arow[i] + ti) & 3));
#pragma unroll
          for (int p = 0; p < P; ++p) af[p][i] = L[p * PATCH + o];
        }
#pragma unroll
        for (int p = 0; p < P; ++p) bfr[p][0] = wb[s][kk * 2 + p];
        mma_half<MI, 1, P, true, NQ, kk>(af, bfr, acc, [&](int q) __attribute__((always_inline)) {
          if (q < 4) {
            gw(t + 2, s2, q);   // past NK: zero-filled, never read
          } else if constexpr (u >= 0) {
            if (more) ppiece(u, (c + 1) & 1);   // the other buffer: last read before the previous barrier
            pload1(u, c + 2);
          }
        });
      });
    });
    __syncthreads();   // the next chunk's patch is stored; this chunk's reads are done
  }
  hs.finish(acc);

  // ---- epilogue from the accumulators: bias, residual, ReLU, max (ximg_kernel's)
  float* out = a.out + (long long)g * a.out_gstride;
  const float* bias = a.bias ? a.bias + (long long)slot * a.b_sstride : nullptr;
  const float* res = a.res ? a.res + (long long)g * a.out_gstride : nullptr;
  float vmax = 0.f;
  const int n = n0 + wn * 32 + fr;
  if (n < a.Ncol) {
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
        if (img0 + m / (W * W) >= nv) continue;
        const long long o = (long long)(img0 * W * W + m) * a.Ncol + n;
        float v = acc[i][0][r];
        if (bias) v += bv;
        if (res) v += res[o];
        if (a.relu) v = relu_nan(v);
        vmax = fmaxf(vmax, fabsf(v));
        out[o] = v;
      }
  }
  if (a.amax_out) amax_fold(a.amax_out, a.amax_out_ld, g, vmax);
}

// the whole-image halo conv: evaluation forward, 3x3 stride-1 pad-1, square W 8 / 4,
// Cs % 32 == 0, no fused BN / lazy operands.  dba_ximg_set: 1 (default) ximg2_kernel where the
// weights carry fragment-ordered planes (ximg_kernel otherwise), 2 ximg_kernel (the bit-equality
// test's and the kernel bench's A/B), 0 off (the tests' A/B against the implicit GEMM)
template <int W, int IMGS, int BN, int WM, int WN>
int ximg_go(const XArgs& a, int G, hipStream_t st) {
  XArgs b = a;
  b.tiles_n = ceil_div(a.Ncol, BN);
  const dim3 grid((unsigned)(ceil_div(a.N, IMGS) * b.tiles_n), G, 1);
  xg::last_launch() = XLast{3, W, BN, a.wp != nullptr, 0, 1, 1, 0};
  if (a.wp) hipLaunchKernelGGL((ximg_kernel<W, IMGS, BN, WM, WN, true>), grid, dim3(256), 0, st, b);
  else hipLaunchKernelGGL((ximg_kernel<W, IMGS, BN, WM, WN, false>), grid, dim3(256), 0, st, b);
  DBA_LAUNCH_CHECK();
}
// ximg_go's grid; -100: the device refuses the two patch buffers (the caller runs ximg_kernel)
template <int W, int IMGS, int BN>
int ximg2_go(const XArgs& a, int G, hipStream_t st) {
  constexpr int PATCH = IMGS * (W + 2) * (W + 2) * 4;
  constexpr int LDS = 2 * 2 * PATCH * (int)sizeof(uint4);
  // the dynamic-LDS attribute is per device (W 4: 73.7 KB, past the 64-KB default)
  static unsigned long long attr_set = 0ull;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -100;
  if (!(attr_set >> dev & 1ull)) {
    if (hipFuncSetAttribute((const void*)ximg2_kernel<W, IMGS, BN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS) != hipSuccess)
      return -100;
    attr_set |= 1ull << dev;
  }
  XArgs b = a;
  b.tiles_n = ceil_div(a.Ncol, BN);
  const dim3 grid((unsigned)(ceil_div(a.N, IMGS) * b.tiles_n), G, 1);
  xg::last_launch() = XLast{4, W, BN, 1, 0, 1, 1, 0};
  hipLaunchKernelGGL((ximg2_kernel<W, IMGS, BN>), grid, dim3(256), LDS, st, b);
  DBA_LAUNCH_CHECK();
}
// ================================================================ 16-wide halo conv, staged weights
// xhalo_kernel<16, 64, 128, 64, 2, 2, PRE> (xhalo.hpp: the evaluation forward of the 16-wide
// stage's plain 64 -> 64 3x3 convs) with the weight path of xblock.hip's GL form: tile, patch, k
// order (tap, then channel block), MFMA sequence per output element and epilogue are that
// kernel's — the same bits — but the B fragments come from the fragment-ordered planes
// (XArgs::wf: k-step index = channel block * 9 + tap) by LDS-DMA.  A weight stage is one tap: its
// two 32-channel k-steps for both 32-column tiles = 16 pieces of 1 KB; wave w copies the 4
// pieces of (column tile w / 2, channel block w % 2), 4 KB contiguous in the planes.  Two stages
// in LDS: 9 barriers instead of 18, the copy in flight for a whole stage (24 MFMAs per wave), no
// VGPR, ds_write or swizzle arithmetic on the weight path, B fragment reads at constant offsets
// off 16 * lane.
// LDS 46,080 (patch) + 32,768 + 1,024 B: two blocks per CU.  The LDS-DMA loads are not
// bounds-checked: xstage16_try admits only whole 64 x 576 fragment planes.
__global__ __launch_bounds__(256) void xstage16_kernel(const XArgs a) {
  constexpr int P = 2, W = 16, CS = 64, BM = 128, BN = 64, WN = 2;
  constexpr int TR = BM / W, PW = W + 2, PR = TR + 2, PP = PR * PW;
  constexpr int CH = CS / 8, PATCH = PP * CH;             // uint4 per plane
  constexpr int TM = 64, TN = 32, MI = TM / 32;
  constexpr int CB = CS / 32;                             // channel blocks (k-steps) per tap
  constexpr int STG = (BN / 32) * CB * 4 * 64;            // uint4 per stage
  static_assert(BM * BN <= P * PATCH * 4, "epilogue tile fits the patch");
  __shared__ __attribute__((aligned(16))) uint4 lds[P * PATCH + 2 * STG];   // patch | two weight stages
  __shared__ long long orow[BM];
  uint4* const patch = lds;
  uint4* const bring = lds + P * PATCH;

  const int g = blockIdx.y;
  const int HT = a.Ho / TR;                               // row tiles per image
  const int tm = blockIdx.x;
  const int img = tm / HT, h0 = (tm - img * HT) * TR;
  if (img >= valid_rows(a.nvalid, g, a.N)) return;
  const int slot = a.wsel ? a.wsel[g] : g;
  const float* __restrict__ src = a.src + (long long)g * a.src_gstride;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int fr = lane & 31, hf = lane >> 5;

  // tap's stage into stage buffer tap & 1: this wave's 4 pieces, 16 B per lane (inline asm: see
  // xblock.hip's fill; the destination is M0 + 16 * lane)
  const uint16_t* F = a.wf + (long long)slot * a.wf_sstride + ((wid >> 1) * (CB * 9) + (wid & 1) * 9) * 2048 + lane * 8;
  auto fill = [&](int tap) __attribute__((always_inline)) {
    const uint32_t dst = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(bring + (tap & 1) * STG + wid * 256));
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(F + tap * 2048 + f * 512), "s"(dst + f * 1024)
                   : "memory");
    }
  };
  auto gl_sync = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  fill(0);

  if (tid < BM)
    orow[tid] = (((long long)img * a.Ho + h0 + tid / W) * a.Wo + tid % W) * a.Ncol;

  // ---- the input patch (xhalo_kernel's): rows h0-1 .. h0+TR, cols -1 .. W, split once
  constexpr int Q4 = CS / 4;
  constexpr int NE = (PP * Q4 + 255) / 256;
  float4 pv[NE];
  {
    const __amdgpu_buffer_rsrc_t rA = rsrc(src, (long long)a.N * a.Hs * a.Ws * CS * 4);
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + 256 * u;
      const int pp = e / Q4, q = e - pp * Q4;
      const int pr = pp / PW, pc = pp - pr * PW;
      const int h = h0 - 1 + pr, w = pc - 1;
      const bool ok = e < PP * Q4 && (unsigned)h < (unsigned)a.Hs && (unsigned)w < (unsigned)a.Ws;
      pv[u] = bload4(rA, ok ? (((img * a.Hs + h) * a.Ws + w) * CS + q * 4) * 4 : kOOB);
    }
  }
  HScale hs;
  hs.init(amax_read(a.amax_src, a.amax_src_ld, g), amax_read(a.amax_w, a.amax_w_ld, slot));
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = tid + 256 * u;
    if (e >= PP * Q4) break;
    const int pp = e / Q4, q = e - pp * Q4;
    uint2 sp[P];
    split4h(pv[u].x, pv[u].y, pv[u].z, pv[u].w, hs.ma, sp);
    const int o = pp * CH + ((q >> 1) ^ hswz<W, CS>(pp, pp % PW));
#pragma unroll
    for (int p = 0; p < P; ++p) ((uint2*)&patch[p * PATCH + o])[q & 1] = sp[p];
  }

  f32x16_t acc[MI][1];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
  int apix[MI], acol[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = wm * TM + i * 32 + fr;
    apix[i] = (m / W) * PW + (m % W);
    acol[i] = m % W;
  }

  // one tap: half-steps h = channel block * 2 + half, fragment set h & 1
  auto stage = [&](int tap) __attribute__((always_inline)) {
    const int ti = tap / 3, tj = tap - ti * 3;
    const int toff = ti * PW + tj;
    const uint4* L = bring + (tap & 1) * STG + wn * (CB * 4 * 64) + lane;
    uint4 af[2][P][MI], bfr[2][P][1];
    auto frags = [&](auto Hc) __attribute__((always_inline)) {
      constexpr int h = decltype(Hc)::value, cb = h / 2, kk = h % 2, st = h & 1;
      const int ch = kk * 2 + hf;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int pp = apix[i] + toff;
        const int o = pp * CH + ((cb * 4 + ch) ^ hswz<W, CS>(pp, acol[i] + tj));
#pragma unroll
        for (int p = 0; p < P; ++p) af[st][p][i] = patch[p * PATCH + o];
      }
#pragma unroll
      for (int p = 0; p < P; ++p) bfr[st][p][0] = L[(cb * 4 + kk * 2 + p) * 64];
    };
    // the next half-step's fragment reads are pinned ahead of this one's MFMAs (left alone, the
    // scheduler sinks each read to just before its MFMA).  eval.layer2, 17 x 1024 images, parent
    // 1153 us: reads sunk 1087, fence behind the MFMAs only 1087, this 1083 us
    // (profiles/r8/xstage/README.md)
    frags(std::integral_constant<int, 0>{});
    sfor<2 * CB>([&](auto Hc) __attribute__((always_inline)) {
      constexpr int h = decltype(Hc)::value;
      if constexpr (h + 1 < 2 * CB) frags(std::integral_constant<int, h + 1>{});
      __builtin_amdgcn_sched_barrier(0);
      mma_half<MI, 1, P, true, 0, h % 2>(af[h & 1], bfr[h & 1], acc, [](int) {});
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  gl_sync();   // patch + the first stage
  for (int tap = 0; tap < 9; ++tap) {
    if (tap + 1 < 9) fill(tap + 1);   // its buffer's last reads ended before the barrier just passed
    stage(tap);
    gl_sync();
  }
  hs.finish(acc);

  // ---- epilogue through the (drained) patch memory (xhalo_kernel's)
  float* Ct = reinterpret_cast<float*>(patch);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      Ct[(wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf) * BN + wn * TN + fr] = acc[i][0][r];
  __syncthreads();
  float* out = a.out + (long long)g * a.out_gstride;
  const float* bias = a.bias ? a.bias + (long long)slot * a.b_sstride : nullptr;
  const float* res = a.res ? a.res + (long long)g * a.out_gstride : nullptr;
  constexpr int C4 = BN / 4;
  float vmax = 0.f;
  for (int e = tid; e < BM * C4; e += 256) {
    const int row = e / C4, n = (e - row * C4) * 4;
    const long long o = orow[row];
    float4 v = *(const float4*)&Ct[row * BN + n];
    if (bias) { v.x += bias[n]; v.y += bias[n + 1]; v.z += bias[n + 2]; v.w += bias[n + 3]; }
    if (res) {
      const float4 rv = *(const float4*)(res + o + n);
      v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
    }
    if (a.relu) relu_nan4(v);
    vmax = fmaxf(vmax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    *(float4*)(out + o + n) = v;
  }
  if (a.amax_out) amax_fold(a.amax_out, a.amax_out_ld, g, vmax);
}

// which kernels take their staged-weight form under dba_xstage_set(1) (each where its kernel-bench
// row beat the parent's by more than three times the parent's run-to-run spread:
// profiles/r8/xstage/README.md)
constexpr bool kXStage16Default = true;

// the staged form takes exactly xhalo_try's W-16 evaluation case with whole fragment planes:
// 3x3 stride-1 pad-1 forward, 16 x 16 x 64 -> 64, pre-split weights, no shortcut / BN / lazy operand
int xstage16_try(const XArgs& a, int G, int KH, int KW, hipStream_t st) {
  const XClass& c = a.cls[0];
  const int mode = xg::xstage_mode();
  if (!(mode == 3 || (mode == 1 && kXStage16Default))) return -100;
  if (KH != 3 || KW != 3 || a.sp != 1 || a.os != 1 || a.dsg != 1 || a.splitk != 1 || c.nI != 3 || c.nJ != 3 ||
      c.bh != -1 || c.bw != -1)
    return -100;
  if (a.Hs != 16 || a.Ws != 16 || a.Ho != 16 || a.Wo != 16 || a.Cs != 64 || a.Ncol != 64) return -100;
  if (a.bf.mode || a.lz_coef || a.sc_src) return -100;
  if (!aligned16(a.src) || !aligned16(a.w) || a.src_gstride % 4 || a.w_sstride % 4) return -100;
  if (!a.wp || !a.wf || ((uintptr_t)a.wf & 15) || a.wf_sstride % 8 || a.wf_sstride < 2 * 64 * 576) return -100;
  xg::last_launch() = XLast{5, 16, 64, 1, 0, 1, 1, 0};
  hipLaunchKernelGGL(xstage16_kernel, dim3((unsigned)(a.N * (a.Ho / 8)), G, 1), dim3(256), 0, st, a);
  DBA_LAUNCH_CHECK();
}

int& ximg_on() {
  static int on = 1;
  return on;
}
int ximg_try(const XArgs& a, int G, int KH, int KW, hipStream_t st) {
  const XClass& c = a.cls[0];
  if (!ximg_on() || KH != 3 || KW != 3 || a.sp != 1 || a.os != 1 || a.dsg != 1 || a.splitk != 1 || c.nI != 3 ||
      c.nJ != 3 || c.bh != -1 || c.bw != -1)
    return -100;
  if (a.Hs != a.Ho || a.Ws != a.Wo || a.Ho != a.Wo || a.Cs % 32 != 0 || a.Ncol % 32 != 0) return -100;
  if (a.bf.mode || a.lz_coef) return -100;
  if (!aligned16(a.src) || a.src_gstride % 4 || !aligned16(a.w) || a.w_sstride % 4) return -100;
  if (a.wp && (((uintptr_t)a.wp & 15) || a.wp_sstride % 8)) return -100;
  if (a.sc_src) return -100;   // the fused shortcut: xhalo_kernel only (see ximg_kernel)
  if (ximg_on() == 1 && a.wp && a.wf && !((uintptr_t)a.wf & 15) && a.wf_sstride % 8 == 0) {
    int rc = -100;
    if (a.Wo == 8) rc = a.Ncol >= 128 ? ximg2_go<8, 2, 128>(a, G, st) : ximg2_go<8, 2, 64>(a, G, st);
    if (a.Wo == 4) rc = a.Ncol >= 128 ? ximg2_go<4, 8, 128>(a, G, st) : ximg2_go<4, 8, 64>(a, G, st);
    if (rc != -100) return rc;
  }
  if (a.Wo == 8) return a.Ncol >= 128 ? ximg_go<8, 2, 128, 2, 2>(a, G, st) : ximg_go<8, 2, 64, 2, 2>(a, G, st);
  if (a.Wo == 4) return a.Ncol >= 128 ? ximg_go<4, 8, 128, 2, 2>(a, G, st) : ximg_go<4, 8, 64, 2, 2>(a, G, st);
  return -100;
}

}  // namespace

// patch-reuse weight gradient (xwgrad_halo.hip) on / off (tests: A/B against the implicit GEMM
// on the same slabs); returns the previous
// the split-K policy (negative: keep); returns 0 (tools / A-B runs: tools.bench_step --split)
DBA_EXPORT int dba_xsplit_policy(int target, int min_k, int max_s, int kslab_max, int dgrad_ks) {
  SplitPolicy& p = split_policy();
  if (dgrad_ks >= 0) p.dgrad_ks = dgrad_ks;
  if (target > 0) p.target = target;
  if (min_k > 0) p.min_k = min_k;
  if (max_s > 0) p.max_s = std::min(max_s, kSkMax);
  if (kslab_max > 0) p.kslab_max = kslab_max;
  return 0;
}

// the last conv-family launch (common.hpp XLast) as 8 ints
DBA_EXPORT int dba_xconv_last_launch(int* out) {
  const XLast& l = xg::last_launch();
  const int v[8] = {l.kind, l.tile, l.vec, l.pre, l.form, l.slabs, l.nclass, l.lazy};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return 0;
}

DBA_EXPORT int dba_ximg_set(int on) {
  const int prev = ximg_on();
  if (on >= 0) ximg_on() = on;
  return prev;
}

// the weight path of the fused evaluation block (xblock.hip) and the 16-wide evaluation conv
// (xstage16_kernel): 1 (default) tap-deep weight stages filled by LDS-DMA from the
// fragment-ordered planes, in each kernel whose default is on and where the weights carry whole
// planes (the ring otherwise); 2 the LDS weight ring (same bits: the bit-equality test's and the
// kernel bench's A/B); 3 the staged form wherever it applies, whatever the kernel's default;
// negative queries.  Returns the previous setting.
DBA_EXPORT int dba_xstage_set(int on) {
  const int prev = xg::xstage_mode();
  if (on >= 1 && on <= 3) xg::xstage_mode() = on;
  return prev;
}

// workspace floats a split-K forward launch of this shape needs (0: none)

DBA_EXPORT long long dba_xconv_ws_floats(int G, int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW) {
  const long long M = (long long)N * Ho * Wo;
  const int s = xsplitk(M, G, Cout, KH * KW * Cin);
  return s > 1 ? (long long)s * G * M * Cout : 0;
}

// arrival counters (int32, zeroed) the in-launch split-K combine of this shape needs (0: it
// does not split, or the combine is off / not applicable: the separate reduce launch runs)

DBA_EXPORT long long dba_xconv_sk_ints(int G, int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW) {
  const long long M = (long long)N * Ho * Wo;
  const int s = xsplitk(M, G, Cout, KH * KW * Cin);
  const long long n = s > 1 ? xconv_sk_count(M, Cout, G, 1, s) : 0;
  return (n > 0 && sk_ok((const int*)1, n, M, Cout, G, 1, s)) ? n : 0;
}

// y = act(conv(x, w) + bias + res), fp32 NHWC; w [slots][Cout][KH][KW][Cin]

DBA_EXPORT int dba_xconv_fwd(const float* x, long long x_gstride, const float* w, long long w_sstride,
                             const int* wsel, const float* bias, long long b_sstride, const float* res, float* out,
                             long long out_gstride, const int* nvalid, int G, int N, int H, int W, int Cin, int Ho,
                             int Wo, int Cout, int KH, int KW, int stride, int pad, int relu, const int* amax_x,
                             int amax_x_ld, const int* amax_w, int amax_w_ld, int* amax_out, int amax_out_ld,
                             const uint16_t* wp, long long wp_sstride, const uint16_t* wf, long long wf_sstride,
                             float* ws, long long ws_floats, int* sk_cnt,
                             long long sk_cnt_n, const void* bnf, const float* lz_coef, int lz_relu,
                             void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if ((long long)N * H * W * Cin >= (1LL << 29)) return -103;   // 32-bit in-replica byte offsets
  const long long M = (long long)N * Ho * Wo;
  const int K = KH * KW * Cin;
  const int vec = (Cin % 4 == 0 && aligned16(x) && aligned16(w) && x_gstride % 4 == 0 && w_sstride % 4 == 0) ? 4 : 1;
  XArgs a{};
  a.src = x; a.src_gstride = x_gstride; a.w = w; a.w_sstride = w_sstride; a.wsel = wsel;
  a.bias = bias; a.b_sstride = b_sstride; a.res = res; a.out = out; a.out_gstride = out_gstride;
  a.nvalid = nvalid; a.N = N; a.Hs = H; a.Ws = W; a.Cs = Cin; a.Ncol = Cout; a.Ho = Ho; a.Wo = Wo;
  a.sp = stride; a.os = 1; a.dsg = 1; a.relu = relu; a.splitk = 1;
  a.amax_src = amax_x; a.amax_w = amax_w; a.amax_out = amax_out;
  a.amax_src_ld = amax_x_ld; a.amax_w_ld = amax_w_ld; a.amax_out_ld = amax_out_ld;
  a.wp = wp; a.wp_sstride = wp_sstride; a.wf = wf; a.wf_sstride = wf_sstride;
  a.cls[0] = XClass{KH, KW, -pad, -pad, 0, 0, Ho, Wo, 0};
  if (!amax_x || !amax_w) return -109;   // the fp16 pair needs both operand maxima
  if (bnf) {
    a.bf = *(const BnFuse*)bnf;
    if (a.bf.mode != 1 || bias || res || relu || (Cout & 3) || a.bf.C != Cout) return -108;
  }
  if (lz_coef) {
    if (wp || vec < 4 || Cin > 512) return -108;
    a.lz_coef = lz_coef; a.lz_relu = lz_relu;
  }
  // a fused BN's finalize launch follows its producer (bnx_tile_go launches its own)
  auto fin = [&](int rc) { return (rc == 0 && a.bf.mode) ? bnx_finalize_go(a.bf, nvalid, G, N, Ho * Wo, st) : rc; };
  if (stride == 1) {
    int rc = ximg_try(a, G, KH, KW, st);
    if (rc == -100) rc = xstage16_try(a, G, KH, KW, st);
    if (rc == -100) rc = xhalo_try(a, G, KH, KW, st);
    if (rc != -100) return fin(rc);
  }
  const int s = xsplitk(M, G, Cout, K);
  const bool ws_ok = s > 1 && ws != nullptr && ws_floats >= (long long)s * G * M * Cout;
  if (s > 1 && !(ws_ok && sk_ok(sk_cnt, sk_cnt_n, M, Cout, G, 1, s))) {
    // grouped launch: the slabs summed inside each block (same bits as the split launches)
    XArgs b = a;
    b.kslab = s;
    const int rc = xconv_ks(b, M, G, vec, st);
    if (rc != -100) return fin(rc);
  }
  if (ws_ok && sk_ok(sk_cnt, sk_cnt_n, M, Cout, G, 1, s)) {
    // in-launch combine (sk_combine): one launch, BN statistics folded by the reducing block
    XArgs b = a;
    b.splitk = s;
    b.zstride = (long long)G * M * Cout;
    b.sk_ws = ws; b.sk_gstride = M * Cout; b.sk_cnt = sk_cnt;
    return fin(xconv_dispatch(b, M, G, 1, vec, st));
  }
  if (ws_ok) {
    XArgs b = a;
    b.splitk = s;
    b.out = ws;
    b.out_gstride = M * Cout;
    b.zstride = (long long)G * M * Cout;
    const int rc = xconv_dispatch(b, M, G, 1, vec, st);
    if (rc != 0) return rc;
    if (a.bf.mode)   // the slabs summed + the statistics in one pass, the epilogue's records (bnfuse.hpp)
      return bnx_tile_go(a.bf, nullptr, out, out_gstride, nvalid, G, N, Ho * Wo, nullptr, 0.f, ws, s, b.zstride,
                         nullptr, st);
    const long long per = M * Cout;
    const dim3 grid((unsigned)std::max(1LL, std::min(1024LL, (per + 255) / 256)), G);
    hipLaunchKernelGGL(xsplitk_reduce_kernel, grid, dim3(256), 0, st, (const float*)ws, s, b.zstride, per, nvalid, N,
                       Ho * Wo, Cout, bias, b_sstride, wsel, res, relu, out, amax_out, amax_out_ld);
    DBA_LAUNCH_CHECK();
  }
  return fin(xconv_dispatch(a, M, G, 1, vec, st));
}

// The conv2 of a downsampling BasicBlock with its 1x1 stride-2 shortcut fused (evaluation, BN
// folded): out = relu(conv3x3(a, w2) + b2 + conv1x1_s2(x2, wsc) + bsc), one launch, the shortcut's
// output never materialised (xhalo_kernel SC: the W-16 stage, 64 channels from 32; 17 x 1024
// images 1348 vs 1886 us for the shortcut conv + the residual-epilogue conv2,
// profiles/r5/down/kbench_ximg_sc.log).  a [G][N][Ho][Wo][C] fp32, x2
// [G][N][H2][W2][C2] fp32 (Ho = ceil(H2 / 2)), w2 / wsc pre-split fp16-pair planes per slot.
// Returns -100 for shapes without a fused kernel (the caller runs the two convs).

DBA_EXPORT int dba_xdown_fwd(const float* a_, long long a_gstride, const float* w2, long long w2_sstride,
                             const uint16_t* w2p, long long w2p_sstride, const int* wsel, const float* b2,
                             long long b_sstride, const float* x2, long long x2_gstride, const uint16_t* wscp,
                             long long wscp_sstride, const float* bsc, long long bsc_sstride, float* out,
                             long long out_gstride, const int* nvalid, int G, int N, int Ho, int Wo, int C, int H2,
                             int W2, int C2, const int* amax_a, int amax_a_ld, const int* amax_w2, int amax_w2_ld,
                             const int* amax_x2, int amax_x2_ld, const int* amax_wsc, int amax_wsc_ld, int* amax_out,
                             int amax_out_ld, void* stream) {
  if (!amax_a || !amax_w2 || !amax_x2 || !amax_wsc || !w2p || !wscp) return -109;
  if ((H2 - 1) / 2 + 1 != Ho || (W2 - 1) / 2 + 1 != Wo || (long long)N * H2 * W2 * C2 >= (1LL << 29) ||
      (long long)N * Ho * Wo * C >= (1LL << 29))
    return -103;
  XArgs a{};
  a.src = a_; a.src_gstride = a_gstride; a.w = w2; a.w_sstride = w2_sstride; a.wsel = wsel;
  a.bias = b2; a.b_sstride = b_sstride; a.res = nullptr; a.out = out; a.out_gstride = out_gstride;
  a.nvalid = nvalid; a.N = N; a.Hs = Ho; a.Ws = Wo; a.Cs = C; a.Ncol = C; a.Ho = Ho; a.Wo = Wo;
  a.sp = 1; a.os = 1; a.dsg = 1; a.relu = 1; a.splitk = 1;
  a.amax_src = amax_a; a.amax_w = amax_w2; a.amax_out = amax_out;
  a.amax_src_ld = amax_a_ld; a.amax_w_ld = amax_w2_ld; a.amax_out_ld = amax_out_ld;
  a.wp = w2p; a.wp_sstride = w2p_sstride;
  a.sc_src = x2; a.sc_gstride = x2_gstride; a.sc_H = H2; a.sc_W = W2; a.sc_C = C2;
  a.sc_wp = wscp; a.sc_wp_sstride = wscp_sstride;
  a.sc_amax_src = amax_x2; a.sc_amax_src_ld = amax_x2_ld; a.sc_amax_w = amax_wsc; a.sc_amax_w_ld = amax_wsc_ld;
  a.sc_bias = bsc; a.sc_b_sstride = bsc_sstride;
  a.cls[0] = XClass{3, 3, -1, -1, 0, 0, Ho, Wo, 0};
  return xhalo_try(a, G, 3, 3, (hipStream_t)stream);
}

// dX of a conv from class-packed transposed weights (dba_xtranspose); accum (optional) is
// added in.  dy [G][N][Ho][Wo][Cout] -> dx [G][N][H][W][Cin]
