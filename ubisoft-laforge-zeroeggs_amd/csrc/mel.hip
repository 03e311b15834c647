// Audio front-end on the GPU: wav -> [n_frames, n_mels + 1] features (log-mel + energy at the animation rate).
//
// Reference (all float64 NumPy): ZEGGS/audio/spectrograms.py:216-269 (symmetric Hann, reflect padding,
// per-frame rfft, |.|/n_fft), :161-183 + :386-443 (Slaney mel filterbank), :57-131 (clip, dB, map to
// [0,1]); ZEGGS/data_pipeline.py:62-80 (10**(x/20) -> ln, linear resampling to the animation rate,
// energy = ||exp(mel)||_2 resampled with extrapolation).
//
// The reference's spectrogram is float64, so everything here computes in float64 as well (MI355X runs f64 FMAs at full vector
// rate).  Three forms of the STFT, same results (float32 features bit-identical, tools/mel_ab.py), chosen from the dims by
// launch_stft: the FFT form mel_stft_fft_k (default: a half-length complex mixed-radix FFT + split, what the reference's
// np.fft.rfft computes), the DFT as a float64 matrix-core product mel_stft_mfma_k (option mel_fft = 0) and the direct DFT
// mel_stft_k (other n_fft).  They differ in how a frame's amplitudes come about; the sample index rule and the window
// (mel_math.h), the per-frame tail (mel_frame_tail), the filterbank's band table (mel_pack_bands) and the float64 feature table
// [STFT frames, n_mels + 1] that the resampling reads (the splines of resample_method = "cubic": spline.h) are stated once.
#include <atomic>
#include <math.h>

#include "../../include/zeggs_hip_live.h"
#include "common.h"
#include "mel_math.h"
#include "spline.h"

namespace {

// the matrix-core form (mel_stft_mfma_k): 32 STFT frames per workgroup
constexpr int MF = 32, MWAVES = 8, MTPW = 7, MCOLP = MWAVES * MTPW * 16;      // frames, waves, column tiles per wave, 896 columns
constexpr int MFB_CAP = 2048;                                                  // filterbank non-zeros staged in LDS
typedef double c2 __attribute__((ext_vector_type(2)));     // (re, im)

// what a call builds once from the dims and the filterbank for the FFT and matrix-core forms (the batched form: zeggs_mel_batch_prepare)
struct MelTables {
  c2* ftw;          // FFT form: [n_fft / 2 + n_fft / 2 + 1 + n_fft] complex (twiddles of the half-length transform, of the split, window)
  double* fbp;      // the filterbank's non-zeros, band after band [MFB_CAP]
  int* bands;       // [3 n_mels] first bin | one past the last bin | offset in fbp
};
MelTables carve_mel_tables(const ZeggsMelDims& d, Arena& a) {
  MelTables t;
  t.ftw = (c2*)a.raw(sizeof(double) * 2 * ((size_t)2 * d.n_fft + 1));
  t.fbp = (double*)a.raw(sizeof(double) * MFB_CAP);
  t.bands = (int*)a.raw(sizeof(int) * 3 * (size_t)d.n_mels);
  return t;
}
struct MelWs {
  double* feat;     // [M, n_mels + 1] log-mel | energy of every STFT frame
  double* table;    // [n_fft, MCOLP]: column 2k = cos(2 pi j k / n_fft), 2k+1 = -sin(.), zero beyond bin n_fft/2
  double* win;      // [n_fft] symmetric Hann
  MelTables t;
  double* spl;      // resample_method = "cubic": second derivatives of the interpolating splines [M, n_mels + 1]
};
MelWs carve_mel(const ZeggsMelDims& d, long M, Arena& a) {
  MelWs w;
  w.feat = (double*)a.raw(sizeof(double) * M * (d.n_mels + 1));
  w.table = (double*)a.raw(sizeof(double) * (size_t)d.n_fft * MCOLP);
  w.win = (double*)a.raw(sizeof(double) * (size_t)d.n_fft);
  w.t = carve_mel_tables(d, a);
  w.spl = (d.flags & MEL_CUBIC) ? (double*)a.raw(sizeof(double) * M * (d.n_mels + 1)) : nullptr;
  return w;
}

// The clipped mel amplitude s -> what the reference stores: v = (20 log10 s + range) / range (spectrograms.py:121-129), then
// data_pipeline.py:62-63 takes y = ln(10^(v / 20)), and the frame's energy is || exp(y) ||_2 (data_pipeline.py:28-30,75).  Four
// float64 transcendentals per mel value (log10, pow, log, exp) bounded the front-end in round 4 (not memory).  Round 5:
//   y = v ln(10) / 20 = ln(s) / range + ln(10) / 20   -- the pow / log pair is an affine map -- and exp(y)^2 = exp(2 y);
//   mode 0: ln(s) and exp(2 y) on the hardware log2 / exp2 (v_log_f32 / v_exp_f32, 1 ulp of float32): the error of y is
//     <= 6e-8 |log2 s| ln 2 / range ~ 1e-8 absolute (range = -20 log10(min amplitude) ~ 10^2), of the energy 1e-7 relative -- the
//     features are float32 and the reference fixtures are matched at 2e-6;
//   mode 2 (default): the affine map in float64 (log10 + exp per value): float32 features bit-identical to mode 1, the literal
//   float64 chain (zeggs_set_option("mel_exact_log", m)).
__device__ __forceinline__ double mel_logamp(double s, double rng, int exact, int flags = 0) {
  if (flags & MEL_RAW_RANGE)      // normalize_range = false: v = 20 log10 s, y = ln(10^(v / 20)) = ln s
    return exact == 0 ? (double)(__builtin_amdgcn_logf((float)s) * 0.6931471805599453f) : exact == 1 ? log(pow(10.0, (20.0 * log10(s)) / 20.0)) : log(s);
  if (exact == 0) return (double)(__builtin_amdgcn_logf((float)s) * 0.6931471805599453f) / rng + (2.302585092994046 / 20.0);
  const double v = (20.0 * log10(s) + rng) / rng;
  return exact == 1 ? log(pow(10.0, v / 20.0)) : v * (2.302585092994046 / 20.0);
}
__device__ __forceinline__ double mel_exp_sq(double y, int exact) {      // exp(y)^2
  if (exact == 0) return (double)__builtin_amdgcn_exp2f((float)(y * (2.0 * 1.4426950408889634)));
  const double z = exp(y);
  return z * z;
}

// Sample `src` (mel_math.h: mel_src) of the signal the STFT sees: the wav, zero where it is not loaded, high-pass filtered first when
// audio_conf.pre_emphasis is on (spectrograms.py:35 -> signal_manipulation.preemphasis = lfilter([1, -c], [1], x): y[n] = x[n] - c x[n-1],
// y[0] = x[0], in float64).  n = signal length for the reflect rule, n_avail = samples present in `wav` (streaming: n is unknown yet and
// passed as a huge value; the caller only asks for frames that end before n_avail); `wav[i]` is sample base + i of the signal (base = 0:
// the whole signal; > 0: a sliding window, zeggs_mel_features_window, whose host side has checked that no frame of the call reads below `base`)
__device__ __forceinline__ double mel_sample(const float* wav, long src, long n, long n_avail, double pe, long base) {
  if (!mel_loaded(src, n, n_avail, base)) return 0.0;
  double x = (double)wav[src - base];
  if (pe != 0.0 && src > base) x -= pe * (double)wav[src - 1 - base];
  return x;
}

// The filterbank's bands, found and packed ONCE per call by one workgroup: bands[m] = first non-zero bin of filter m, bands[NM + m] = one
// past its last, bands[2 NM + m] = offset of the band in fbp (-1: does not fit MFB_CAP, read from the dense matrix) -- every STFT workgroup
// copies these few KB into LDS instead of scanning the dense [n_mels, n_bins] matrix itself (that scan was 2/3 of the FFT form's first
// version's time).  All threads walk the dense matrix together (min / max through global atomics on the band table itself: a serial scan
// per filter was 0.13 ms of a 1.7 ms front-end).
__device__ void mel_pack_bands(const double* fb, int NM, int NBIN, int* bands, double* fbp) {
  for (int m = threadIdx.x; m < NM; m += blockDim.x) { bands[m] = NBIN; bands[NM + m] = 0; }
  __syncthreads();
  for (int i = threadIdx.x; i < NM * NBIN; i += blockDim.x) {
    const int m = i / NBIN, k = i - m * NBIN;
    if (fb[i] != 0.0) { atomicMin(bands + m, k); atomicMax(bands + NM + m, k + 1); }
  }
  __syncthreads();
  for (int m = threadIdx.x; m < NM; m += blockDim.x)
    if (bands[NM + m] == 0) bands[m] = 0;            // an all-zero filter: empty band [0, 0)
  __syncthreads();
  if (threadIdx.x == 0) {
    int o = 0;
    for (int m = 0; m < NM; ++m) {
      const int w = bands[NM + m] - bands[m];
      if (o + w <= MFB_CAP) { bands[2 * NM + m] = o; o += w; } else bands[2 * NM + m] = -1;
    }
  }
  __syncthreads();
  for (int m = threadIdx.x; m < NM; m += blockDim.x)
    if (bands[2 * NM + m] >= 0)
      for (int k = bands[m]; k < bands[NM + m]; ++k) fbp[bands[2 * NM + m] + k - bands[m]] = fb[(long)m * NBIN + k];
}
// ... and a workgroup's copy of them: fbs [MFB_CAP], blo [3 NM] in LDS (first bin | one past the last | offset, contiguous)
__device__ __forceinline__ void mel_stage_bands(const int* bands, const double* fbp, int NM, double* fbs, int* blo) {
  for (int i = threadIdx.x; i < 3 * NM; i += blockDim.x) blo[i] = bands[i];
  for (int i = threadIdx.x; i < MFB_CAP; i += blockDim.x) fbs[i] = fbp[i];
}

// The per-frame tail of all three forms: amplitudes amp [F][n_bins] of F STFT frames in LDS (written, and a barrier passed) -> rows
// slot0 .. slot0 + F - 1 of the feature table (those below nfr are stored): mel band sum, |.|, clip, log chain, and in column n_mels the
// energy || exp(log-mel) ||_2 (data_pipeline.py:28-30,75).  Filter m adds its band in bin order, from the staged non-zeros fbs where it
// has an offset, from the dense matrix fb otherwise; blo == nullptr (the direct form builds no band table): the whole dense row, which
// gives the same bits -- fma(0, a, s) == s for finite a, and s starts at +0.  esq [F][n_mels]: LDS scratch apart from amp.  Every thread
// takes the exponential of its own value; the frame's thread only adds, in mel order.
__device__ __forceinline__ void mel_frame_tail(const ZeggsMelDims& d, int F, const double* amp, double* esq, const int* blo, const double* fbs,
                                               const double* fb, double* feat, long slot0, long nfr, int exact) {
  const int NF = d.n_fft, NBIN = NF / 2 + 1, NM = d.n_mels, W = NM + 1, tid = threadIdx.x;
  const int* bhi = blo != nullptr ? blo + NM : nullptr;
  const int* bof = blo != nullptr ? blo + 2 * NM : nullptr;
  const double amin = (double)d.min_clip / (double)NF;  // spectrograms.py:88-90
  const double rng = -20.0 * log10(amin);
  for (int it = tid; it < F * NM; it += blockDim.x) {
    const int f = it / NM, m = it % NM;
    const double* av = amp + (size_t)f * NBIN;
    double s = 0.0;
    if (blo != nullptr && bof[m] >= 0) {
      const double* fv = fbs + bof[m] - blo[m];
      for (int k = blo[m]; k < bhi[m]; ++k) s = fma(fv[k], av[k], s);
    } else {
      const double* fv = fb + (long)m * NBIN;
      const int lo = blo != nullptr ? blo[m] : 0, hi = blo != nullptr ? bhi[m] : NBIN;
      for (int k = lo; k < hi; ++k) s = fma(fv[k], av[k], s);
    }
    s = fabs(s);
    if (s < amin) s = amin;
    const double y = mel_logamp(s, rng, exact, d.flags);
    esq[it] = mel_exp_sq(y, exact);
    if (slot0 + f < nfr) feat[(slot0 + f) * W + m] = y;
  }
  __syncthreads();
  if (tid < F && slot0 + tid < nfr) {
    double e = 0.0;
    for (int m = 0; m < NM; ++m) e += esq[tid * NM + m];
    feat[(slot0 + tid) * W + NM] = sqrt(e);
  }
}

// ---- direct DFT (mel_stft_k): one workgroup per STFT frame m0 + blockIdx.x, the windowed frame and an n_fft-entry cos/sin table are
// staged in LDS, each thread evaluates a direct DFT for its bins (index k*n mod n_fft walks the table, no trigonometry in the loop)
__global__ __launch_bounds__(256) void mel_stft_k(ZeggsMelDims d, const float* wav, long n, long n_avail, const double* fb, double* feat,
                                                   long m0, int exact, long base) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int NF = d.n_fft, NBIN = NF / 2 + 1;
  double* xw = sm;              // [NF] windowed samples
  double* ct = xw + NF;         // [NF] cos(2 pi j / NF)
  double* st = ct + NF;         // [NF] sin
  double* amp = st + NF;        // [NBIN]
  double* esq = amp + NBIN;     // [n_mels]
  const long fr = m0 + blockIdx.x, slot = blockIdx.x;
  for (int j = threadIdx.x; j < NF; j += blockDim.x) {
    xw[j] = mel_sample(wav, mel_src(d, fr, j, n), n, n_avail, d.pre_emph, base) * mel_hann(j, NF);
    const double ang = 2.0 * M_PI * (double)j / (double)NF;
    ct[j] = cos(ang);
    st[j] = sin(ang);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < NBIN; k += blockDim.x) {
    double re = 0.0, im = 0.0;
    int idx = 0;
    for (int j = 0; j < NF; ++j) {
      const double x = xw[j];
      re = fma(x, ct[idx], re);
      im = fma(-x, st[idx], im);
      idx += k;
      if (idx >= NF) idx -= NF;
    }
    amp[k] = sqrt(re * re + im * im) / (double)NF;     // real_amplitude (spectrograms.py:266-267)
  }
  __syncthreads();
  mel_frame_tail(d, 1, amp, esq, nullptr, nullptr, fb, feat, slot, slot + 1, exact);
}

// ---- matrix-core DFT (mel_stft_mfma_k): 32 STFT frames per workgroup, the DFT as a [frames, n_fft] x [n_fft, 2 bins] fp64
// product on v_mfma_f64_16x16x4_f64 against a cos / -sin table built once per call
typedef double d4 __attribute__((ext_vector_type(4)));

// DFT basis + window, once per call (the angle is reduced exactly: (j k) mod n_fft -- the same table entries the direct
// kernel above walks); block 0 also packs the filterbank's bands
__global__ void mel_table_k(double* T, double* win, int NF, int NBIN, const double* fb, int NM, int* bands, double* fbp) {
  const long n = (long)NF * MCOLP;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i / MCOLP), c = (int)(i % MCOLP), k = c >> 1;
    double v = 0.0;
    if (k < NBIN) {
      const double ang = 2.0 * M_PI * (double)(((long)j * k) % NF) / (double)NF;
      v = (c & 1) ? -sin(ang) : cos(ang);
    }
    T[i] = v;
    if (i < NF) win[i] = mel_hann((int)i, NF);
  }
  if (blockIdx.x == 0) mel_pack_bands(fb, NM, NBIN, bands, fbp);
}

// LDS of mel_stft_mfma_k (bytes): raw samples of the 32 overlapping frames | window | amplitudes [32][NBIN] | staged filterbank
// non-zeros | band tables.  The tail's scratch reuses the sample area after the products.
__host__ __device__ inline size_t mel_fast_lds(int NF, int hop, int n_mels) {
  const size_t ns = (size_t)(MF - 1) * hop + NF;
  size_t xs = ns * sizeof(float), mv = (size_t)MF * n_mels * sizeof(double);
  if (mv > xs) xs = mv;
  xs = (xs + 15) / 16 * 16;
  return xs + sizeof(double) * ((size_t)NF + (size_t)MF * (NF / 2 + 1) + MFB_CAP) + sizeof(int) * 3 * (size_t)n_mels + 64;
}

// STFT frames m0 + 32 blockIdx.x ... (nfr frames in all): same results as mel_stft_k -- identical table entries, window and tail;
// only the n_fft-term DFT sums are accumulated by the matrix cores (fp64, k in steps of 4) instead of one fma chain per bin.
// It stages raw float32 samples (launch_stft sends pre-emphasis elsewhere).
__global__ __launch_bounds__(MWAVES * 64) void mel_stft_mfma_k(ZeggsMelDims d, const float* wav, long n, long n_avail,
                                                                const double* fb, const double* table, const double* wintab,
                                                                const int* bands, const double* fbp, double* feat, long m0, long nfr,
                                                                int exact, long base) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int NF = d.n_fft, NBIN = NF / 2 + 1, hop = d.hop, NM = d.n_mels;
  const int ns = (MF - 1) * hop + NF;
  size_t xs_bytes = (size_t)ns * sizeof(float), mv_bytes = (size_t)MF * NM * sizeof(double);
  if (mv_bytes > xs_bytes) xs_bytes = mv_bytes;
  xs_bytes = (xs_bytes + 15) / 16 * 16;
  float* xs = (float*)smem;                         // [ns] samples (reflect rule applied)
  double* esq = (double*)smem;                      // [MF][NM] after the products
  double* win = (double*)(smem + xs_bytes);         // [NF]
  double* amp = win + NF;                           // [MF][NBIN]
  double* fbs = amp + (size_t)MF * NBIN;            // [MFB_CAP]
  int* blo = (int*)(fbs + MFB_CAP);                 // [3 NM]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long fr0 = m0 + (long)blockIdx.x * MF, slot0 = (long)blockIdx.x * MF;
  for (int i = tid; i < ns; i += blockDim.x) {      // (tap i of frame fr0 = tap i - f hop of frame fr0 + f)
    const long src = mel_src(d, fr0, i, n);
    xs[i] = mel_loaded(src, n, n_avail, base) ? wav[src - base] : 0.f;
  }
  for (int j = tid; j < NF; j += blockDim.x) win[j] = wintab[j];
  mel_stage_bands(bands, fbp, NM, fbs, blo);
  __syncthreads();
  // ---- DFT: P[frame][col] = sum_j xw[frame][j] T[j][col]; this wave: column tiles wave * MTPW .. + MTPW - 1, both row tiles
  d4 acc[2][MTPW];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int t = 0; t < MTPW; ++t) acc[rt][t] = d4{0.0, 0.0, 0.0, 0.0};
  const int r16 = lane & 15, kk = lane >> 4;
  const double* tb = table + (long)kk * MCOLP + 16 * (wave * MTPW) + r16;
  double bq[MTPW];
#pragma unroll
  for (int t = 0; t < MTPW; ++t) bq[t] = tb[16 * t];
  for (int s4 = 0; s4 < NF; s4 += 4) {
    const int j = s4 + kk;
    const double wj = win[j];
    const double a0 = (double)xs[r16 * hop + j] * wj, a1 = (double)xs[(16 + r16) * hop + j] * wj;
    double bc[MTPW];
#pragma unroll
    for (int t = 0; t < MTPW; ++t) bc[t] = bq[t];
    if (s4 + 4 < NF) {
      const double* tn = tb + (long)(s4 + 4) * MCOLP;
#pragma unroll
      for (int t = 0; t < MTPW; ++t) bq[t] = tn[16 * t];
    }
#pragma unroll
    for (int t = 0; t < MTPW; ++t) {
      acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bc[t], acc[0][t], 0, 0, 0);
      acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bc[t], acc[1][t], 0, 0, 0);
    }
  }
  // accumulator layout of the f64 form: col = lane & 15, row = (lane >> 4) + 4 i.  Even column = Re, odd = Im of bin col / 2
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int t = 0; t < MTPW; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double v = acc[rt][t][i];
        const double o = __shfl_xor(v, 1, 64);
        const int col = 16 * (wave * MTPW + t) + r16, bin = col >> 1, fr = rt * 16 + kk + 4 * i;
        if (!(col & 1) && bin < NBIN) amp[(size_t)fr * NBIN + bin] = sqrt(v * v + o * o) / (double)NF;   // real_amplitude
      }
  __syncthreads();
  mel_frame_tail(d, MF, amp, esq, blo, fbs, fb, feat, slot0, nfr, exact);      // (esq is the sample area: the products are done)
}


// ---- FFT form (mel_stft_fft_k, round 4): what the reference's np.fft.rfft does (spectrograms.py:251-263) instead of the
// O(N^2) DFT as a matrix product -- an n_fft-point real transform as ONE complex FFT of half the length (even samples real part,
// odd samples imaginary part), mixed-radix Stockham autosort in LDS (radices 4 / 5 / 2: 400 = 4 4 5 5 for the shipped
// n_fft = 800), then the usual split X[k] = (Z[k] + conj Z[M-k]) / 2 - i / 2 e^{-2 pi i k / N} (Z[k] - conj Z[M-k]).
// 19 kFLOP per STFT frame instead of 1.28 MFLOP; the launch is bound by the log / exp chain of the 80 mel values and by LDS
// traffic, not by the transform.  Twiddles come from two tables built once per call in float64 (exact angle reduction), so
// the spectrum agrees with the matrix form to a few ulp.
constexpr int FFB = 4;            // STFT frames per workgroup
constexpr int FTHR = 320;          // 5 waves: the radix-5 stages (4 x 80 butterflies) and the mel / log chain (4 x 80 values) are ONE pass each
constexpr int FMAXST = 8;         // stages
struct FftPlan { int nst; int radix[FMAXST]; };
__device__ __forceinline__ c2 cmul(c2 a, c2 b) { return c2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ c2 cmul_mi(c2 a) { return c2{a.y, -a.x}; }      // a * (-i)

// TW[n] = exp(-2 pi i n / M), n < M;  TW[M + k] = exp(-2 pi i k / (2 M)), k <= M;  TW[2 M + 1 + j] = (hann window j, 0), j < 2 M.
// Block 0 also packs the filterbank's bands.
__global__ void mel_fft_table_k(c2* TW, int M, const double* fb, int NM, int* bands, double* fbp) {
  const int NF = 2 * M, n = 2 * M + 1 + NF;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i < M) { const double a = 2.0 * M_PI * (double)i / (double)M; TW[i] = c2{cos(a), -sin(a)}; }
    else if (i <= 2 * M) { const double a = 2.0 * M_PI * (double)(i - M) / (double)NF; TW[i] = c2{cos(a), -sin(a)}; }
    else TW[i] = c2{mel_hann(i - 2 * M - 1, NF), 0.0};
  }
  if (blockIdx.x == 0) mel_pack_bands(fb, NM, M + 1, bands, fbp);
}

__host__ __device__ inline size_t mel_fft_lds(int NF, int n_mels) {
  return sizeof(double) * 2 * ((size_t)2 * FFB * (NF / 2)) + sizeof(double) * MFB_CAP + sizeof(int) * 3 * (size_t)n_mels + 64;
}

// One workgroup's share: STFT frames fr0 .. fr0 + FFB - 1 of ONE signal -> feature rows slot0 .. (those below nfr are
// stored).  The body of mel_stft_fft_k and of mel_stft_fft_batch_k: one statement of the per-frame arithmetic for both.
__device__ __forceinline__ void mel_stft_fft_frames(const ZeggsMelDims& d, const FftPlan& plan, const float* wav, long n, long n_avail,
                                                    const double* fb, const MelTables& tab, double* feat, const long fr0,
                                                    const long slot0, long nfr, int exact, long base, unsigned char* smem) {
  const int NF = d.n_fft, M = NF / 2, NBIN = M + 1, NM = d.n_mels;
  const c2* __restrict__ TW = tab.ftw;
  c2* bufA = (c2*)smem;                               // [FFB][M]
  c2* bufB = bufA + (size_t)FFB * M;                  // [FFB][M]
  double* fbs = (double*)(bufB + (size_t)FFB * M);    // [MFB_CAP]
  int* blo = (int*)(fbs + MFB_CAP);                   // [3 NM]
  const int tid = threadIdx.x;
  const c2* WIN = TW + 2 * M + 1;
  // windowed samples, packed: z[m] = xw[2 m] + i xw[2 m + 1]
  for (int i = tid; i < FFB * M; i += blockDim.x) {
    const int f = i / M, m = i - f * M;
    double v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * m + h;
      v[h] = mel_sample(wav, mel_src(d, fr0 + f, j, n), n, n_avail, d.pre_emph, base) * WIN[j].x;
    }
    bufA[i] = c2{v[0], v[1]};
  }
  mel_stage_bands(tab.bands, tab.fbp, NM, fbs, blo);
  __syncthreads();
  // ---- Stockham stages: x -> y, natural order in, natural order out
  c2* x = bufA;
  c2* y = bufB;
  int Ns = 1;
  for (int st = 0; st < plan.nst; ++st) {
    const int r = plan.radix[st], t = M / r, tws = M / (Ns * r);      // tws: table stride of this stage's twiddle
    for (int it = tid; it < FFB * t; it += blockDim.x) {
      const int f = it / t, i = it - f * t;
      const int k = i % Ns, j = (i - k) * r + k;
      const c2* xi = x + (size_t)f * M + i;
      c2* yo = y + (size_t)f * M + j;
      if (r == 4) {
        c2 u0 = xi[0], u1 = xi[t], u2 = xi[2 * t], u3 = xi[3 * t];
        if (k) { const int a = k * tws; u1 = cmul(u1, TW[a]); u2 = cmul(u2, TW[2 * a]); u3 = cmul(u3, TW[3 * a]); }
        const c2 s0 = u0 + u2, s1 = u0 - u2, s2 = u1 + u3, s3 = cmul_mi(u1 - u3);
        yo[0] = s0 + s2; yo[Ns] = s1 + s3; yo[2 * Ns] = s0 - s2; yo[3 * Ns] = s1 - s3;
      } else if (r == 5) {
        c2 u0 = xi[0], u1 = xi[t], u2 = xi[2 * t], u3 = xi[3 * t], u4 = xi[4 * t];
        if (k) {
          const int a = k * tws;
          u1 = cmul(u1, TW[a]); u2 = cmul(u2, TW[2 * a]); u3 = cmul(u3, TW[3 * a]); u4 = cmul(u4, TW[4 * a]);
        }
        const double c1 = 0.30901699437494742, c2_ = -0.80901699437494742;      // cos(2 pi / 5), cos(4 pi / 5)
        const double s1 = 0.95105651629515357, s2 = 0.58778525229247313;        // sin(2 pi / 5), sin(4 pi / 5)
        const c2 a1 = u1 + u4, a2 = u2 + u3, b1 = u1 - u4, b2 = u2 - u3;
        const c2 m1 = u0 + c1 * a1 + c2_ * a2, m2 = u0 + c2_ * a1 + c1 * a2;
        const c2 n1 = cmul_mi(s1 * b1 + s2 * b2), n2 = cmul_mi(s2 * b1 - s1 * b2);       // -i (...)
        yo[0] = u0 + a1 + a2; yo[Ns] = m1 + n1; yo[2 * Ns] = m2 + n2; yo[3 * Ns] = m2 - n2; yo[4 * Ns] = m1 - n1;
      } else {      // r == 2
        c2 u0 = xi[0], u1 = xi[t];
        if (k) u1 = cmul(u1, TW[k * tws]);
        yo[0] = u0 + u1; yo[Ns] = u0 - u1;
      }
    }
    __syncthreads();
    c2* tmp = x; x = y; y = tmp;
    Ns *= r;
  }
  // ---- split: amplitude of bin k of the real transform (real_amplitude: |X[k]| / n_fft) -> the other buffer
  double* amp = (double*)y;                           // [FFB][NBIN] doubles <= [FFB][M] complex
  for (int it = tid; it < FFB * NBIN; it += blockDim.x) {
    const int f = it / NBIN, k = it - f * NBIN;
    const c2* Z = x + (size_t)f * M;
    const c2 zk = Z[k == M ? 0 : k], zm = Z[k == 0 ? 0 : M - k];
    const c2 zc = c2{zm.x, -zm.y};
    const c2 xe = 0.5 * (zk + zc), dd = 0.5 * (zk - zc);
    const c2 xo = c2{dd.y, -dd.x};                    // (zk - conj zm) / (2 i)
    const c2 X = xe + cmul(TW[M + k], xo);
    amp[(size_t)f * NBIN + k] = sqrt(X.x * X.x + X.y * X.y) / (double)NF;
  }
  __syncthreads();
  mel_frame_tail(d, FFB, amp, (double*)x, blo, fbs, fb, feat, slot0, nfr, exact);      // (the spectrum buffer is free now)
}

__global__ __launch_bounds__(FTHR) void mel_stft_fft_k(ZeggsMelDims d, FftPlan plan, const float* wav, long n, long n_avail,
                                                      const double* fb, MelTables tab, double* feat, long m0, long nfr, int exact,
                                                      long base) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  mel_stft_fft_frames(d, plan, wav, n, n_avail, fb, tab, feat, m0 + (long)blockIdx.x * FFB, (long)blockIdx.x * FFB, nfr, exact,
                      base, smem);
}

// The batched form (zeggs_mel_features_batch): workgroup b works on row r with blk0[r] <= b < blk0[r + 1], block b - blk0[r] of that
// row's nfr[r] STFT frames m0[r] ..; a row's feature rows are [r S, r S + nfr[r]) of one table.  What the host derived per row travels by
// value (1.5 KB); the records themselves (pointers, counts) are read from device memory, wave-uniformly.
struct MelBatchPlan {
  int blk0[ZEGGS_LIVE_MAX_ROWS + 1];
  int nfr[ZEGGS_LIVE_MAX_ROWS];
  long m0[ZEGGS_LIVE_MAX_ROWS];
  long M[ZEGGS_LIVE_MAX_ROWS];       // STFT frames of the finished signal (final) or 2^40
};
__global__ __launch_bounds__(FTHR) void mel_stft_fft_batch_k(ZeggsMelDims d, FftPlan plan, const ZeggsMelRow* __restrict__ rows,
                                                            MelBatchPlan bp, int R, long S, const double* fb, MelTables tab,
                                                            double* feat, int exact) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int r = 0;
  while (r + 1 < R && (int)blockIdx.x >= bp.blk0[r + 1]) ++r;
  const long blk = (long)((int)blockIdx.x - bp.blk0[r]);
  const float* wav = rows[r].wav;
  const long n_avail = rows[r].n_samples, base = rows[r].base;
  const long n = rows[r].final ? n_avail : (1L << 50);
  mel_stft_fft_frames(d, plan, wav, n, n_avail, fb, tab, feat + (size_t)r * S * (d.n_mels + 1), bp.m0[r] + blk * FFB, blk * FFB,
                      (long)bp.nfr[r], exact, base, smem);
}

// resampling at t_k = mel_rate k.  "linear" / "cubic": mel -> NaN outside the hull (griddata's fill value), the energy extrapolates
// (interp1d(fill_value = "extrapolate"): the end pieces continue); "nearest": both take the nearest frame, halves round DOWN, ends clamp
// (interp1d's bounds x_i + 1/2 searched from the left; griddata sets fill_value = "extrapolate" for this method).
// one element: column c (mel channel, or the energy at c == n_mels) of animation frame k; feat / spl indexed by ABSOLUTE STFT frame
__device__ __forceinline__ float mel_resample_elem(const ZeggsMelDims& d, const double* feat, const double* spl, long M, int c, long k) {
  const int W = d.n_mels + 1;
  const double t = mel_rate(d) * (double)k;
  if (d.flags & MEL_NEAREST) {
    long q = (long)ceil(t - 0.5);
    q = q < 0 ? 0 : q > M - 1 ? M - 1 : q;
    return (float)feat[q * W + c];
  }
  long hi = (long)ceil(t);            // searchsorted(side=left) over the integer grid
  if (hi < 1) hi = 1;
  if (hi > M - 1) hi = M - 1;
  const long lo = hi - 1;
  if (M < 2) return nanf("");
  if (c < d.n_mels && (t < 0.0 || t > (double)(M - 1))) return nanf("");
  const double ylo = feat[lo * W + c], yhi = feat[hi * W + c];
  if (d.flags & MEL_CUBIC) return (float)spline_piece(ylo, yhi, spl[lo * W + c], spl[hi * W + c], t - (double)lo);
  return (float)((yhi - ylo) * (t - (double)lo) + ylo);
}
// animation frames k0 .. k0 + n_frames - 1; feat holds the STFT frames m0 .. (rows relative to m0)
__global__ void mel_resample_k(ZeggsMelDims d, const double* feat, const double* spl, long M, long m0, long k0, int n_frames, float* out) {
  const int W = d.n_mels + 1;
  const long n = (long)n_frames * W;
  feat -= m0 * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = mel_resample_elem(d, feat, spl, M, (int)(i % W), k0 + i / W);
}
// the batched sibling: blockIdx.y = row; M, m0 (plan) and k0, the frame count and the output (record) are the row's own
__global__ void mel_resample_batch_k(ZeggsMelDims d, const ZeggsMelRow* __restrict__ rows, MelBatchPlan bp, long S, const double* feat) {
  const int W = d.n_mels + 1, r = blockIdx.y;
  const long k0 = rows[r].k0, n = (rows[r].k1 - k0) * W;
  float* out = rows[r].out;
  feat += ((long)r * S - bp.m0[r]) * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = mel_resample_elem(d, feat, nullptr, bp.M[r], (int)(i % W), k0 + i / W);
}

}  // namespace

int g_mel_mfma = 1;      // zeggs_set_option("mel_mfma", 0/1): matrix-core DFT / one workgroup per frame, direct DFT (when the FFT form is off)
int g_mel_exact_log = 2;      // zeggs_set_option("mel_exact_log", 0 / 1 / 2): see mel_logamp (measured on 30 min of audio: 1.61 / 1.50 / 1.46 ms for
                              // modes 1 / 2 / 0 -- the transcendentals are NOT what bounds the kernel; mode 2 equals the literal chain bit for bit in float32)
int g_mel_fft = 1;       // zeggs_set_option("mel_fft", 0/1): the FFT form (default; n_fft / 2 must factor into 4, 5, 2)

// radices of the half-length transform: 4s first, then 5s, then a 2 (400 = 4 4 5 5); nst = 0: not this path
static FftPlan fft_plan(int M) {
  FftPlan p{};
  int m = M, n4 = 0, n5 = 0, n2 = 0;
  while (m % 4 == 0) { m /= 4; ++n4; }
  while (m % 5 == 0) { m /= 5; ++n5; }
  while (m % 2 == 0) { m /= 2; ++n2; }
  if (m != 1 || n4 + n5 + n2 > FMAXST || n4 + n5 + n2 == 0) return p;
  for (int i = 0; i < n4; ++i) p.radix[p.nst++] = 4;
  for (int i = 0; i < n5; ++i) p.radix[p.nst++] = 5;
  for (int i = 0; i < n2; ++i) p.radix[p.nst++] = 2;
  return p;
}

thread_local int t_mel_launches = 0;      // kernels enqueued by this thread's range / window / batch calls (zeggs_mel_batch_last_ops)
thread_local int t_mel_form = 0;          // the STFT form this thread enqueued last (zeggs_mel_last_form): set where t_mel_launches is bumped
constexpr size_t MEL_LDS_MAX = 160 * 1024;      // dynamic LDS a workgroup may be given (with the per-kernel opt-in above 64 KB)

// The opt-in, once per kernel and process; `done` is that kernel's flag.  Two threads that arrive together both set the attribute (it
// is idempotent); neither launches before its own call has returned.
static int mel_lds_opt_in(const void* kernel, std::atomic<bool>& done, const char* who, const char* name) {
  if (done.load(std::memory_order_acquire)) return 0;
  ZCHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MEL_LDS_MAX) == hipSuccess,
         "%s: cannot raise the LDS limit of the %s kernel", who, name);
  done.store(true, std::memory_order_release);
  return 0;
}

// whether the FFT form takes these dimensions (and the option allows it); *plan: its radices
static bool mel_fft_form(const ZeggsMelDims& d, FftPlan* plan) {
  *plan = fft_plan(d.n_fft / 2);
  return g_mel_fft && plan->nst > 0 && d.n_fft % 2 == 0 && mel_fft_lds(d.n_fft, d.n_mels) <= MEL_LDS_MAX &&
         (size_t)FFB * d.n_mels <= (size_t)2 * FFB * (d.n_fft / 2);
}

// STFT frames m0 .. m0 + nfr - 1 -> rows 0 .. nfr - 1 of w.feat
// (`base`: index of wav[0] in the signal, see mel_sample)
static int launch_stft(const ZeggsMelDims& d, const MelWs& w, const float* wav, long n, long n_avail, const double* fb, long m0,
                       long nfr, hipStream_t s, long base = 0) {
  const int NBIN = d.n_fft / 2 + 1;
  FftPlan plan;
  if (mel_fft_form(d, &plan) && nfr >= 1) {
    static std::atomic<bool> opted{false};
    ZTRY(mel_lds_opt_in((const void*)mel_stft_fft_k, opted, "mel", "FFT"));
    hipLaunchKernelGGL(mel_fft_table_k, dim3(16), dim3(256), 0, s, w.t.ftw, d.n_fft / 2, fb, d.n_mels, w.t.bands, w.t.fbp);
    ZLAUNCH_CHECK("mel_fft_table");
    hipLaunchKernelGGL(mel_stft_fft_k, dim3((unsigned)((nfr + FFB - 1) / FFB)), dim3(FTHR), mel_fft_lds(d.n_fft, d.n_mels), s, d, plan, wav, n,
                       n_avail, fb, w.t, w.feat, m0, nfr, g_mel_exact_log, base);
    ZLAUNCH_CHECK("mel_stft_fft");
    t_mel_launches += 2;
    t_mel_form = 1;
    return 0;
  }
  const size_t fast_lds = mel_fast_lds(d.n_fft, d.hop, d.n_mels);
  if (g_mel_mfma && d.pre_emph == 0.0 && d.n_fft % 4 == 0 && 2 * NBIN <= MCOLP && fast_lds <= MEL_LDS_MAX && nfr >= 1) {   // (stages float32 samples)
    static std::atomic<bool> opted{false};
    ZTRY(mel_lds_opt_in((const void*)mel_stft_mfma_k, opted, "mel", "matrix-core"));
    hipLaunchKernelGGL(mel_table_k, dim3(1024), dim3(256), 0, s, w.table, w.win, d.n_fft, NBIN, fb, d.n_mels, w.t.bands, w.t.fbp);
    ZLAUNCH_CHECK("mel_table");
    hipLaunchKernelGGL(mel_stft_mfma_k, dim3((unsigned)((nfr + MF - 1) / MF)), dim3(MWAVES * 64), fast_lds, s, d, wav, n, n_avail,
                       fb, w.table, w.win, w.t.bands, w.t.fbp, w.feat, m0, nfr, g_mel_exact_log, base);
    ZLAUNCH_CHECK("mel_stft_mfma");
    t_mel_launches += 2;
    t_mel_form = 2;
    return 0;
  }
  // the direct form takes what the other two decline; its frame, cos / sin table, amplitudes and mel values live in LDS, which ends it
  // (n_fft <= 5828 at 80 mel channels; from 2318 on it is past the 64 KB a kernel gets without the opt-in) -- refused here, ahead of the launch
  const size_t lds = sizeof(double) * (3 * (size_t)d.n_fft + d.n_fft / 2 + 1 + d.n_mels);
  ZCHECK(lds <= MEL_LDS_MAX, "mel: n_fft = %d with %d mel channels needs %zu bytes of LDS per STFT frame, a workgroup has %zu", d.n_fft,
         d.n_mels, lds, MEL_LDS_MAX);
  static std::atomic<bool> opted{false};
  ZTRY(mel_lds_opt_in((const void*)mel_stft_k, opted, "mel", "direct"));
  hipLaunchKernelGGL(mel_stft_k, dim3((unsigned)nfr), dim3(256), lds, s, d, wav, n, n_avail, fb, w.feat, m0, g_mel_exact_log, base);
  ZLAUNCH_CHECK("mel_stft");
  t_mel_launches += 1;
  t_mel_form = 3;
  return 0;
}

extern "C" long zeggs_mel_stft_frames(const ZeggsMelDims* d, long n_samples) {
  return stft_frames(n_samples, d->n_fft, d->hop, d->flags);
}

extern "C" size_t zeggs_mel_workspace_bytes(const ZeggsMelDims* d, long n_samples) {
  Arena a(nullptr, 0);
  carve_mel(*d, stft_frames(n_samples, d->n_fft, d->hop, d->flags), a);
  return a.off + 256;
}

extern "C" int zeggs_mel_features(const ZeggsMelDims* dp, const float* wav, long n_samples, const double* filterbank,
                                  int n_frames, float* out, void* ws, size_t ws_bytes, void* stream) {
  const ZeggsMelDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  ZCHECK(d.n_fft >= 2 && d.n_fft % 2 == 0 && d.hop > 0 && d.n_mels > 0, "mel: bad dims");
  ZCHECK(n_samples > 0 && n_frames >= 0, "mel: empty input");
  const long M = stft_frames(n_samples, d.n_fft, d.hop, d.flags);
  Arena a(ws, ws_bytes);
  MelWs w = carve_mel(d, M, a);
  ZCHECK(a.ok(), "mel: workspace too small (%zu < %zu)", ws_bytes, a.off);
  ZTRY(launch_stft(d, w, wav, n_samples, n_samples, filterbank, 0L, M, s));
  if (n_frames > 0) {
    long n = (long)n_frames * (d.n_mels + 1), g = (n + 255) / 256;
    if (d.flags & MEL_CUBIC) {      // one spline per column of the feature table over the WHOLE signal
      ZCHECK(M >= 4, "mel: resample_method \"cubic\" needs at least 4 STFT frames (got %ld)", M);      // (scipy raises the same way)
      spline_second_derivatives(w.feat, M, d.n_mels + 1, w.spl, s);
      ZLAUNCH_CHECK("mel_spline");
    }
    hipLaunchKernelGGL(mel_resample_k, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, d, w.feat, w.spl, M, 0L, 0L, n_frames, out);
    ZLAUNCH_CHECK("mel_resample");
  }
  return 0;
}

// Streaming form: features of the animation frames [k0, k1) from the samples received so far.
//   final == 0: the signal continues; every STFT frame the range needs must end inside the n_samples present
//               (zeggs_mel_frames_ready tells how far that is) -- no right-edge reflection, no end clamps;
//   final != 0: n_samples is the whole signal: identical to rows k0..k1-1 of zeggs_mel_features.
extern "C" long zeggs_mel_frames_ready(const ZeggsMelDims* d, long n_samples) { return mel_frames_ready(*d, n_samples); }
extern "C" size_t zeggs_mel_range_workspace_bytes(const ZeggsMelDims* d, long k0, long k1) {
  Arena a(nullptr, 0);
  carve_mel(*d, mel_range_slots(*d, k0, k1), a);
  return a.off + 256;
}
constexpr long MEL_M_OPEN = 1L << 40, MEL_N_OPEN = 1L << 50;      // STFT frames / samples of a signal that continues
extern "C" long zeggs_mel_window_first_sample(const ZeggsMelDims* d, long k0) {
  long m0, m1;
  mel_range_stft(*d, MEL_M_OPEN, k0, k0 + 1, &m0, &m1);
  const long f = mel_first_load(*d, m0, m1, MEL_N_OPEN, MEL_N_OPEN);      // (the signal continues: no right end)
  return f == __LONG_MAX__ ? 0 : f;
}
// the argument checks of a range / window call, ahead of any launch (`who`: "" or the batched call's "mel batch: row r: ");
// -> the STFT frames [m0, m1) the range interpolates and M
static int mel_range_check(const ZeggsMelDims& d, long base, long n_samples, int final, long k0, long k1, const char* who, long* M,
                           long* m0, long* m1) {
  ZCHECK(d.n_fft >= 2 && d.n_fft % 2 == 0 && d.hop > 0 && d.n_mels > 0, "%smel: bad dims", who);
  ZCHECK(n_samples > 0 && k0 >= 0 && k1 > k0, "%smel range: empty input", who);
  ZCHECK(!(d.flags & MEL_CUBIC), "%smel range: resample_method \"cubic\" is a spline over the WHOLE signal -- use zeggs_mel_features", who);
  if (!final)
    ZCHECK(k1 <= mel_frames_ready(d, n_samples), "%smel range: frames %ld..%ld need samples not received yet", who, k0, k1);
  *M = final ? stft_frames(n_samples, d.n_fft, d.hop, d.flags) : MEL_M_OPEN;
  mel_range_stft(d, *M, k0, k1, m0, m1);
  if (base > 0) {
    const long first = mel_first_load(d, *m0, *m1, final ? n_samples : MEL_N_OPEN, n_samples);
    ZCHECK(base <= first, "%smel window: frames %ld..%ld read sample %ld, the window starts at %ld", who, k0, k1, first, base);
  }
  return 0;
}
static int mel_range_impl(const ZeggsMelDims* dp, const float* wav, long base, long n_samples, int final, const double* filterbank,
                          long k0, long k1, float* out, void* ws, size_t ws_bytes, void* stream) {
  const ZeggsMelDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  long M, m0, m1;
  ZTRY(mel_range_check(d, base, n_samples, final, k0, k1, "", &M, &m0, &m1));
  const long n = final ? n_samples : MEL_N_OPEN;
  Arena a(ws, ws_bytes);
  MelWs w = carve_mel(d, m1 - m0, a);
  ZCHECK(a.ok(), "mel range: workspace too small (%zu < %zu)", ws_bytes, a.off);
  ZTRY(launch_stft(d, w, wav, n, n_samples, filterbank, m0, m1 - m0, s, base));
  const long nn = (k1 - k0) * (d.n_mels + 1), g = (nn + 255) / 256;
  hipLaunchKernelGGL(mel_resample_k, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, d, w.feat, nullptr, M, m0, k0, (int)(k1 - k0), out);
  ZLAUNCH_CHECK("mel_resample");
  t_mel_launches += 1;
  return 0;
}
extern "C" int zeggs_mel_features_range(const ZeggsMelDims* dp, const float* wav, long n_samples, int final,
                                        const double* filterbank, long k0, long k1, float* out, void* ws, size_t ws_bytes,
                                        void* stream) {
  return mel_range_impl(dp, wav, 0, n_samples, final, filterbank, k0, k1, out, ws, ws_bytes, stream);
}
// The same rows from a sliding window of the signal: wav_window[i] is sample base + i, n_samples the ABSOLUTE count received so
// far (the window holds samples base .. n_samples - 1).  Refused when a frame of the range would load a sample below `base`
// (zeggs_mel_window_first_sample(d, k0) while the signal continues; with final != 0 the right-end reflection is looked at too).
// Workspace: zeggs_mel_range_workspace_bytes(d, k0, k1).
extern "C" int zeggs_mel_features_window(const ZeggsMelDims* dp, const float* wav_window, long base, long n_samples, int final,
                                         const double* filterbank, long k0, long k1, float* out, void* ws, size_t ws_bytes,
                                         void* stream) {
  ZCHECK(base >= 0 && base < n_samples, "mel window: the window [%ld, %ld) is empty", base, n_samples);
  return mel_range_impl(dp, wav_window, base, n_samples, final, filterbank, k0, k1, out, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- batched form (include/zeggs_hip_live.h)
namespace {
struct MelBatchWs { ZeggsMelRow* rows; double* feat; void* row_ws; size_t row_ws_bytes; };
// records | feature table of all rows, S slots each; the fall-back's per-row workspace shares the second region (the rows run one after another)
MelBatchWs carve_mel_batch(const ZeggsMelDims& d, int R, long S, Arena& a) {
  MelBatchWs w;
  w.rows = (ZeggsMelRow*)a.raw(sizeof(ZeggsMelRow) * ZEGGS_LIVE_MAX_ROWS);
  const size_t mark = align_up(a.off, 256);
  w.feat = (double*)a.raw(sizeof(double) * (size_t)R * S * (d.n_mels + 1));
  const size_t end = a.off;
  Arena b(nullptr, 0);
  carve_mel(d, S, b);
  w.row_ws = a.dry ? nullptr : (void*)(a.base + mark);
  w.row_ws_bytes = b.off;
  if (mark + b.off > end) a.off = mark + b.off;
  return w;
}
}  // namespace

extern "C" size_t zeggs_mel_batch_tables_bytes(const ZeggsMelDims* d) {
  Arena a(nullptr, 0);
  carve_mel_tables(*d, a);
  return a.off + 256;
}

extern "C" int zeggs_mel_batch_prepare(const ZeggsMelDims* dp, const double* filterbank, void* tables, size_t bytes, void* stream) {
  const ZeggsMelDims& d = *dp;
  ZCHECK(d.n_fft >= 2 && d.n_fft % 2 == 0 && d.hop > 0 && d.n_mels > 0, "mel: bad dims");
  Arena a(tables, bytes);
  MelTables t = carve_mel_tables(d, a);
  ZCHECK(tables != nullptr && filterbank != nullptr && a.ok(), "mel batch: table buffer too small (%zu < %zu)", bytes, a.off);
  hipLaunchKernelGGL(mel_fft_table_k, dim3(16), dim3(256), 0, (hipStream_t)stream, t.ftw, d.n_fft / 2, filterbank, d.n_mels, t.bands, t.fbp);
  ZLAUNCH_CHECK("mel_fft_table");
  return 0;
}

extern "C" size_t zeggs_mel_batch_workspace_bytes(const ZeggsMelDims* d, int rows, long max_frames_per_row) {
  Arena a(nullptr, 0);
  carve_mel_batch(*d, rows, mel_batch_slots(*d, max_frames_per_row), a);
  return a.off + 256;
}

extern "C" int zeggs_mel_batch_last_ops() { return t_mel_launches; }
extern "C" int zeggs_mel_last_form(void) { return t_mel_form; }

extern "C" int zeggs_mel_features_batch(const ZeggsMelDims* dp, const ZeggsMelRow* rows, const ZeggsMelRow* rows_dev, int R,
                                        const double* filterbank, const void* tables, void* ws, size_t ws_bytes, void* stream) {
  const ZeggsMelDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  t_mel_launches = 0;
  ZCHECK(R >= 1 && R <= ZEGGS_LIVE_MAX_ROWS, "mel batch: %d rows (1..%d)", R, ZEGGS_LIVE_MAX_ROWS);
  ZCHECK(rows != nullptr && filterbank != nullptr && tables != nullptr && ws != nullptr, "mel batch: NULL argument");
  ZCHECK(d.n_fft >= 2 && d.n_fft % 2 == 0 && d.hop > 0 && d.n_mels > 0, "mel: bad dims");
  // ---- every row's checks, all ahead of any launch
  MelBatchPlan bp{};
  long maxF = 0, max_elems = 0;
  int live = 0;
  for (int r = 0; r < R; ++r) {
    const ZeggsMelRow& w = rows[r];
    char who[40];
    snprintf(who, sizeof who, "mel batch: row %d: ", r);
    bp.blk0[r + 1] = bp.blk0[r];
    ZCHECK(w.k0 >= 0 && w.k1 >= w.k0, "%sframes %ld..%ld", who, w.k0, w.k1);
    if (w.k1 == w.k0) continue;      // the row takes no part
    ZCHECK(w.wav != nullptr && w.out != nullptr, "%sNULL window or output", who);
    ZCHECK(w.base >= 0 && w.base < w.n_samples, "%smel window: the window [%ld, %ld) is empty", who, w.base, w.n_samples);
    long m1;
    ZTRY(mel_range_check(d, w.base, w.n_samples, w.final, w.k0, w.k1, who, &bp.M[r], &bp.m0[r], &m1));
    bp.nfr[r] = (int)(m1 - bp.m0[r]);
    bp.blk0[r + 1] = bp.blk0[r] + (bp.nfr[r] + FFB - 1) / FFB;
    if (w.k1 - w.k0 > maxF) maxF = w.k1 - w.k0;
    ++live;
  }
  const long S = mel_batch_slots(d, maxF);
  Arena a(ws, ws_bytes);
  MelBatchWs w = carve_mel_batch(d, R, S, a);
  ZCHECK(a.off + 256 <= ws_bytes, "mel batch: workspace too small (%zu < %zu)", ws_bytes, a.off + 256);
  for (int r = 0; r < R; ++r) ZCHECK(bp.nfr[r] <= S, "mel batch: row %d: %d STFT frames in %ld slots", r, bp.nfr[r], S);
  if (live == 0) return 0;
  FftPlan plan;
  if (!mel_fft_form(d, &plan)) {      // the per-row path, row after row (each call checks its row again)
    for (int r = 0; r < R; ++r) {
      const ZeggsMelRow& q = rows[r];
      if (q.k1 == q.k0) continue;
      ZTRY(mel_range_impl(dp, q.wav, q.base, q.n_samples, q.final, filterbank, q.k0, q.k1, q.out, w.row_ws, w.row_ws_bytes, stream));
    }
    return 0;
  }
  static std::atomic<bool> opted{false};      // (per kernel: mel_stft_fft_k's own opt-in does not cover this one)
  ZTRY(mel_lds_opt_in((const void*)mel_stft_fft_batch_k, opted, "mel batch", "FFT"));
  if (rows_dev == nullptr) {
    if (hipMemcpyAsync(w.rows, rows, sizeof(ZeggsMelRow) * R, hipMemcpyHostToDevice, s) != hipSuccess) {
      zeggs_set_error("mel batch: cannot upload the row records");
      return -1;
    }
    rows_dev = w.rows;
    ++t_mel_launches;
  }
  Arena ta((void*)tables, (size_t)1 << 40);
  const MelTables t = carve_mel_tables(d, ta);
  hipLaunchKernelGGL(mel_stft_fft_batch_k, dim3((unsigned)bp.blk0[R]), dim3(FTHR), mel_fft_lds(d.n_fft, d.n_mels), s, d, plan, rows_dev, bp,
                     R, S, filterbank, t, w.feat, g_mel_exact_log);
  ZLAUNCH_CHECK("mel_stft_fft_batch");
  for (int r = 0; r < R; ++r) {
    const long e = (rows[r].k1 - rows[r].k0) * (d.n_mels + 1);
    if (e > max_elems) max_elems = e;
  }
  const long g = (max_elems + 255) / 256;
  hipLaunchKernelGGL(mel_resample_batch_k, dim3((unsigned)(g > 64 ? 64 : g), (unsigned)R), dim3(256), 0, s, d, rows_dev, bp, S,
                     (const double*)w.feat);
  ZLAUNCH_CHECK("mel_resample_batch");
  t_mel_launches += 2;
  t_mel_form = 4;
  return 0;
}
