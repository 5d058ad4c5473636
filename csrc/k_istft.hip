// iSTFTNet head (Kaneko et al., ICASSP 2022, C8C8I): the generator's last stage as an inverse STFT.
//
//   lrelu(0.01) -> reflect pad (one row, left) -> Conv1d(C -> n_fft + 2, k = 7, pad 3) -> exp / sin ->
//   16-point inverse real DFT, periodic Hann window -> overlap-add (hop 4) / window envelope -> [int16]
//
// One workgroup (4 waves) owns the samples [4 t0, 4 (t0 + BM)) of one utterance (istft_index.h):
//   1. stage the rows behind the padded positions [t0 - 4, t0 + BM + 4] into LDS as stored (bf16; position 0
//      is row 1, positions outside 0..T are zeros);
//   2. the conv for the frames [t0 - 1, t0 + BM + 1] on v_mfma_f32_16x16x32_bf16: M = frames, K = 7 C,
//      N = 18 padded to 32.  lrelu(x) = max(x, 0) + slope * min(x, 0), and both parts are exact in bf16 where
//      slope * x is not, so each A fragment is split by sign in registers and feeds two accumulators that are
//      joined in fp32: the operands are exactly the stored x and w, only the fp32 accumulation rounds.  The
//      wave grid is 2 (K halves) x 2 (frame halves); a wave's B fragments (its K half of the bf16 weight image
//      [18][7][C]) are loaded once, straight from global memory into registers, and stay there;
//   3. the two K halves meet in LDS in a fixed order (+ bias); exp, sin, cos, the 16 x 9 synthesis and the
//      window run in fp32 on the VALU (libm-grade expf / sinf / cosf: the numerics bound decides, not speed);
//   4. overlap-add of the <= 4 covering frames in ascending frame order from LDS, divided by the envelope of
//      istft_index.h, written as fp32 or clamped int16.
// No atomics, no scratch: every sample is written once by one thread, from sums in a fixed order, so an
// utterance's samples do not depend on its neighbours in the batch and two runs are bitwise equal.
#include "common.h"
#include "istft_index.h"

namespace {

constexpr int IH_NT = 256;  // threads per workgroup
constexpr int IH_BM = 128;  // tile rows

// cos(2 pi m / 16), m = 0..15; sin(2 pi m / 16) = cos(2 pi (m - 4) / 16)
__device__ const float IH_COS16[16] = {1.f,  0.92387953f,  0.70710678f,  0.38268343f,  0.f, -0.38268343f,
                                       -0.70710678f, -0.92387953f, -1.f, -0.92387953f, -0.70710678f, -0.38268343f,
                                       0.f,  0.38268343f,  0.70710678f,  0.92387953f};

template <int C, int NFFT, int HOP>
struct IH {
  static_assert(NFFT == 16 && HOP == 4, "istft head: n_fft 16 / hop 4");
  static_assert(C % 64 == 0, "istft head: a K step of 32 stays inside one tap and K splits in two");
  static constexpr int NB = NFFT / 2 + 1;                            // bins
  static constexpr int NO = NFFT + 2;                                // conv outputs
  static constexpr int BM = IH_BM;
  static constexpr int NFR = istft_tile_frames(BM, NFFT, HOP);       // frames of a tile
  static constexpr int NPOS = istft_tile_positions(BM, NFFT, HOP);   // staged positions
  static constexpr int MT = (NFR + 15) / 16;                         // 16-frame MFMA row tiles
  static constexpr int MTH = (MT + 1) / 2;                           // row tiles per frame half
  static constexpr int XROWS = MT * 16 + ISTFT_TAPS - 1;             // slots the A fragments may touch
  static constexpr int PITCH = 2 * C + 16;                           // bytes per slot (row + one 16-B pad)
  static constexpr int KPT = C / 32;                                 // K steps per tap
  static constexpr int NKS = ISTFT_TAPS * KPT;                       // K steps
  static constexpr int KPH = NKS / 2;                                // per K half
  static constexpr int XBYTES = XROWS * PITCH;
  static constexpr int PBYTES = 2 * MT * 16 * NO * 4;                // the K halves' partial sums
  static constexpr int SPEC = MT * 16 * NB * 8;                      // {re, im} per frame and bin (aliases x)
  static constexpr int FRB = MT * 16 * NFFT * 4;                     // windowed frames (aliases x, after SPEC)
  static constexpr int LDS = XBYTES + PBYTES;
  static_assert(NKS % 2 == 0, "K halves");
  static_assert(SPEC + FRB <= XBYTES, "spectrum and frames alias the x tile");
  static_assert(LDS <= 64 * 1024, "istft head tile");
};

template <int C, int NFFT, int HOP>
__global__ void __launch_bounds__(IH_NT) istft_head_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wimg,
                                                           const float* __restrict__ bias, int Tp, float slope,
                                                           float scale, float* __restrict__ outf,
                                                           int16_t* __restrict__ outi, const int4* __restrict__ tt,
                                                           long ostride) {
  using G = IH<C, NFFT, HOP>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::LDS];
  // padded: block (x, y) = tile x of row y of [B, Tp, C], its samples at out[y * ostride + n]; packed: tt[block] =
  // {first row of the sequence in x, its rows, t0, sequence} (k_vocoder.hip TileGeo), a null tile has rows = 0
  int T, t0;
  long xo, oo;
  if (tt) {
    const int4 e = tt[blockIdx.x];
    xo = e.x;
    T = e.y;
    t0 = e.z;
    oo = (long)e.w * ostride;
  } else {
    T = Tp;
    t0 = blockIdx.x * G::BM;
    xo = (long)blockIdx.y * Tp;
    oo = (long)blockIdx.y * ostride;
  }
  if (T < 2 || t0 < 0 || t0 >= T) return;  // null tile (or nothing to own): loads and stores nothing
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int kh = wave & 1, mh = wave >> 1;

  // this wave's B fragments: k steps kh * KPH .. + KPH - 1, output channels col and 16 + col (>= NO: zeros)
  short8 bfr[G::KPH][2];
#pragma unroll
  for (int i = 0; i < G::KPH; ++i) {
    const int k0 = (kh * G::KPH + i) * 32 + 8 * quad;
    bfr[i][0] = *reinterpret_cast<const short8*>(wimg + (long)col * (ISTFT_TAPS * C) + k0);
    bfr[i][1] = short8{0, 0, 0, 0, 0, 0, 0, 0};
    if (16 + col < G::NO) bfr[i][1] = *reinterpret_cast<const short8*>(wimg + (long)(16 + col) * (ISTFT_TAPS * C) + k0);
  }

  // 1. rows behind the positions p0 .. p0 + NPOS - 1, 16 B per lane; the slots beyond are zeros too (the last
  //    row tile's spare frames read them)
  const bf16_t* xb = x + xo * C;
  const int p0 = istft_tile_pos0(t0, NFFT, HOP);
  constexpr int CH = C / 8;
  for (int e = tid; e < G::XROWS * CH; e += IH_NT) {
    const int s = e / CH, q = e % CH;
    const int r = s < G::NPOS ? istft_pos_row(p0 + s, T) : -1;
    short8 v = short8{0, 0, 0, 0, 0, 0, 0, 0};
    if (r >= 0) v = *reinterpret_cast<const short8*>(xb + (long)r * C + q * 8);
    *reinterpret_cast<short8*>(lds + s * G::PITCH + q * 16) = v;
  }
  __syncthreads();

  // 2. frame fl (local) tap t reads slot fl + t
  float* part = reinterpret_cast<float*>(lds + G::XBYTES);  // [2][MT * 16][NO]
  const int mt1 = (mh + 1) * G::MTH < G::MT ? (mh + 1) * G::MTH : G::MT;
  for (int mt = mh * G::MTH; mt < mt1; ++mt) {
    float4v ap[2], an[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) ap[s] = an[s] = float4v{0.f, 0.f, 0.f, 0.f};
    const unsigned char* abase = lds + (mt * 16 + col) * G::PITCH + 16 * quad;
#pragma unroll
    for (int i = 0; i < G::KPH; ++i) {
      const int ks = kh * G::KPH + i;  // kh is wave-uniform; tap and channel offset follow at run time
      const int tap = ks / G::KPT, c0 = (ks % G::KPT) * 32;
      const uint4 raw = *reinterpret_cast<const uint4*>(abase + tap * G::PITCH + c0 * 2);
      const uint32_t d[4] = {raw.x, raw.y, raw.z, raw.w};
      uint32_t dp[4], dn[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t m = ((d[j] >> 15) & 0x00010001u) * 0xFFFFu;  // 0xFFFF in each half whose sign bit is set
        dn[j] = d[j] & m;
        dp[j] = d[j] & ~m;
      }
      union {
        uint32_t u[4];
        short8 v;
      } fp, fn;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        fp.u[j] = dp[j];
        fn.u[j] = dn[j];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        ap[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp.v, bfr[i][s], ap[s], 0, 0, 0);
        an[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fn.v, bfr[i][s], an[s], 0, 0, 0);
      }
    }
    // C/D: column = lane & 15, row = 4 * (lane >> 4) + r
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int n = s * 16 + col;
      if (n < G::NO) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          part[(kh * G::MT * 16 + mt * 16 + 4 * quad + r) * G::NO + n] = ap[s][r] + slope * an[s][r];
      }
    }
  }
  __syncthreads();  // the x tile is dead from here on

  // 3a. {c_k mag cos(phi), c_k mag sin(phi)} per frame and bin
  float2* spec = reinterpret_cast<float2*>(lds);                  // [MT * 16][NB]
  float* fr = reinterpret_cast<float*>(lds + G::SPEC);            // [MT * 16][NFFT]
  const float* part1 = part + G::MT * 16 * G::NO;
  for (int e = tid; e < G::NFR * G::NB; e += IH_NT) {
    const int fl = e / G::NB, k = e % G::NB;
    const float zm = (part[fl * G::NO + k] + part1[fl * G::NO + k]) + bias[k];
    const float zp = (part[fl * G::NO + G::NB + k] + part1[fl * G::NO + G::NB + k]) + bias[G::NB + k];
    const float mag = expf(zm) * ((k == 0 || k == G::NB - 1) ? 1.f : 2.f);
    const float phi = sinf(zp);
    spec[e] = make_float2(mag * cosf(phi), mag * sinf(phi));
  }
  __syncthreads();
  // 3b. frame[n] = win[n] / N * sum_k re_k cos(2 pi k n / N) - im_k sin(2 pi k n / N)
  for (int e = tid; e < G::NFR * NFFT; e += IH_NT) {
    const int fl = e / NFFT, n = e % NFFT;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < G::NB; ++k) {
      const int m = (k * n) & (NFFT - 1);
      const float2 v = spec[fl * G::NB + k];
      s += v.x * IH_COS16[m];
      s -= v.y * IH_COS16[(m + 12) & 15];
    }
    fr[e] = s * (istft_hann16(n) * (1.f / NFFT));
  }
  __syncthreads();

  // 4. overlap-add over the covering frames of 0..T, ascending, / envelope
  const int fr0 = istft_tile_frame0(t0, NFFT, HOP);
  const int nb = istft_tile_sample_begin(t0, HOP), ne = istft_tile_sample_end(t0, G::BM, T, HOP);
  for (int n = nb + tid; n < ne; n += IH_NT) {
    const int f0 = istft_first_frame(n, NFFT, HOP), f1 = istft_last_frame(n, NFFT, HOP, T);
    float s = 0.f;
    for (int f = f0; f <= f1; ++f) s += fr[(f - fr0) * NFFT + (n + NFFT / 2 - HOP * f)];
    const float y = s / istft_env16(n, HOP, T);
    if (outi) {
      float v = y * scale;
      v = fminf(fmaxf(v, -32768.f), 32767.f);
      outi[oo + n] = (int16_t)v;
    } else {
      outf[oo + n] = y;
    }
  }
}

template <int C>
int launch_istft(dim3 grid, const bf16_t* x, const bf16_t* wimg, const float* b, int T, float slope, float scale,
                 float* outf, int16_t* outi, const int4* tt, long ostride, hipStream_t s) {
  hipLaunchKernelGGL((istft_head_kernel<C, 16, 4>), grid, dim3(IH_NT), 0, s, x, wimg, b, T, slope, scale, outf, outi,
                     tt, ostride);
  return (int)hipGetLastError();
}

}  // namespace

// x [B, T, C] bf16, wimg the bf16 [18][7][C] image of the conv_post weight, b fp32 [18] -> out [B, 4 T] (fp32, or
// int16 = clamp(y * scale)).  -1: no kernel for this C / n_fft / hop; -2: T < 2 (the reflection needs two rows).
SSAMD_API int ssamd_istft_head(const bf16_t* x, const bf16_t* wimg, const float* b, int B, int T, int C, int n_fft,
                               int hop, float slope, float scale, float* outf, int16_t* outi, hipStream_t s) {
  if (n_fft != 16 || hop != 4) return -1;
  if (B <= 0) return 0;
  if (T < 2) return -2;
  if (!b || (long)T * hop >= 2147483647L) return -3;
  dim3 grid(cdiv(T, IH_BM), B);
  switch (C) {
    case 128: return launch_istft<128>(grid, x, wimg, b, T, slope, scale, outf, outi, nullptr, (long)T * hop, s);
    case 64: return launch_istft<64>(grid, x, wimg, b, T, slope, scale, outf, outi, nullptr, (long)T * hop, s);
    default: return -1;
  }
}

// Packed rows x [R, C]: tt = ntt tiles of ssamd_istft_head_tile_rows() rows, sample n of sequence u written to
// out[u * ostride + n] (the caller zero-fills the samples past each length).
SSAMD_API int ssamd_istft_head_pk(const bf16_t* x, const bf16_t* wimg, const float* b, const int* tt, int ntt, int C,
                                  int n_fft, int hop, float slope, float scale, float* outf, int16_t* outi,
                                  long ostride, hipStream_t s) {
  if (n_fft != 16 || hop != 4) return -1;
  if (ntt <= 0) return 0;
  if (!tt) return -2;
  if (!b) return -3;
  const int4* t4 = reinterpret_cast<const int4*>(tt);
  switch (C) {
    case 128: return launch_istft<128>(dim3(ntt), x, wimg, b, 0, slope, scale, outf, outi, t4, ostride, s);
    case 64: return launch_istft<64>(dim3(ntt), x, wimg, b, 0, slope, scale, outf, outi, t4, ostride, s);
    default: return -1;
  }
}

SSAMD_API int ssamd_istft_head_tile_rows() { return IH_BM; }

// 1 when istft_head_kernel is instantiated for this geometry
SSAMD_API int ssamd_istft_head_has(int C, int n_fft, int hop) {
  return (n_fft == 16 && hop == 4 && (C == 128 || C == 64)) ? 1 : 0;
}
