// Spectrum analysis of synthesized audio: what the editor's interactive window shows while the user moves its sliders
// (gama_tts_editor/src/interactive/AnalysisWindow.cpp:189-300, showData; :303-361, setupWindow).  There every output sample
// also goes into a ring of 65 536 samples (InteractiveAudio.cpp:146-158, 192-205; MAX_NUM_SAMPLES_FOR_ANALYSIS,
// InteractiveAudio.h:40), and each full ring becomes one picture.
//
// The rule, for one buffer s[0 .. 65536) of float samples, a window of W doubles (W a power of two in [32, 65536]):
//   1. peak      maxValue = the largest |s[i]| over all 65 536 samples (not only the window's).  maxValue > 0: normCoef =
//                (float)(1.0 / (double)maxValue) and s[i] = s[i] * normCoef, one float product; maxValue == 0: s stays.
//   2. signal    the first W normalised samples, unwindowed.
//   3. spectrum  x[i] = (float)((double)s[i] * window[i]) for i < W, 0 behind (signal_ is float, window_ double:
//                AnalysisWindow.h:72-76); X = rDFT_65536(x) in float (SignalDFT.h:55-68); mag[i] = sqrt(re^2 + im^2) / 256
//                (sqrt(1.0 / 65536) is 2^-8, so the factor is exact); linear: mag[i]; log: 20 log10(mag[i]), min_db where
//                that is below min_db (log10(0) = -inf, so an empty bin is min_db); the bins 0 .. n_bins - 1, n_bins the
//                first i with i * ((double)sample_rate / 65536) > max_freq, else 32 769 (max_freq <= 0: all of them).
//   4. buffers   an utterance's buffers are consecutive and complete, as the ring hands them over: buffer k is the samples
//                [first + 65536 k, first + 65536 (k + 1)); min(max_buffers, floor((count - first) / 65536)) of them are
//                analysed, none if first > count.
// The window scales what it sends to the ring by a running peak.  Step 1 removes any constant scale, so the entries take
// the unscaled samples the synthesis entries write.
//
// This header is the one text of steps 1 to 4 for the host's restatement and the device's lanes (built without FMA
// contraction: step 1 and the window product are single rounded operations), and of the float transform's butterflies,
// which the kernels of vtm_analysis.hip run a thread at a time.  The float transform is not the reference's FFTW bit for
// bit (float DFTs differ by factorisation); the yardstick of both sides is the double DFT of the same x.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/gama_vtm.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GVTM_ANALYSIS_HD __host__ __device__ inline
#else
#include <cmath>
#define GVTM_ANALYSIS_HD inline
#endif

namespace gvtm {

constexpr int kAnalysisSize = GVTM_ANALYSIS_FFT_SIZE;  // FFT_SIZE = MAX_NUM_SAMPLES_FOR_ANALYSIS
constexpr int kAnalysisHalf = kAnalysisSize / 2;       // the complex transform the real one is folded into
constexpr int kAnalysisBins = GVTM_ANALYSIS_MAX_BINS;

// ---- design (vtm_design.cpp; double, this machine's libm) ----

// AnalysisWindow::setupWindow's five formulas; false for a type it does not know
bool design_analysis_window(int type, unsigned size, std::vector<double>& out);
// the first bin whose frequency lies above max_freq (showData's loop, :284-290); max_freq <= 0: every bin
size_t design_analysis_bin_count(unsigned sample_rate, double max_freq);
// W_65536^k = (cos, -sin)(2 pi k / 65536) for k in [0, 32768), each rounded once from double: 2 x 32768 floats
void design_analysis_twiddles(std::vector<float>& out);

// ---- steps 1 to 4 ----

GVTM_ANALYSIS_HD int64_t analysis_buffer_count(int64_t count, int64_t first, int64_t max_buffers)
{
	if (first < 0 || first > count || max_buffers <= 0) return 0;
	const int64_t full = (count - first) / kAnalysisSize;
	return full < max_buffers ? full : max_buffers;
}

// (1.0f where the buffer is silent: the product then leaves every sample as it is)
GVTM_ANALYSIS_HD float analysis_norm_coef(float max_value)
{
	return max_value > 0.0f ? static_cast<float>(1.0 / static_cast<double>(max_value)) : 1.0f;
}

GVTM_ANALYSIS_HD float analysis_normalised(float s, float norm_coef)
{
	return s * norm_coef;
}

GVTM_ANALYSIS_HD float analysis_windowed(float normalised, double window)
{
	return static_cast<float>(static_cast<double>(normalised) * window);
}

// what is shown for a bin of magnitude mag (already scaled by 1/256)
// A bin that is no number (a NaN or an infinity among the window's samples, a peak so small that normCoef is inf) is shown
// as the one quiet NaN 0x7fc00000, linear or log: IEEE 754 leaves the sign of a NaN result to the lanes, and the host's
// make ffc00000 of inf - inf where the device's make 7fc00000, so without this the same text gave other bits on either.
GVTM_ANALYSIS_HD float analysis_level(float mag, bool log_scale, float min_db)
{
	if (mag != mag) return __builtin_nanf("");
	if (!log_scale) return mag;
	const float db = 20.0f * log10f(mag);
	return db < min_db ? min_db : db; // (-inf: an empty bin is min_db)
}

// ---- the float transform ----
// 65 536 real points are the 32 768-point complex transform of z[n] = x[2n] + i x[2n+1] and an untangling pass; the
// complex transform is split 128 x 256 (n = n1 + 128 n2, k = 256 k1 + k2):
//   A  for 16 columns n1 at a time, 256-point transforms over n2, times W_32768^(n1 k2), to T[k2][n1]
//   B  for 32 rows k2 at a time, 128-point transforms over n1, to Z[256 k1 + k2]
//   C  X[k] = (Z[k] + conj Z[M-k]) / 2 - i W_65536^k (Z[k] - conj Z[M-k]) / 2, its magnitude and level
// The sub-transforms are Stockham radix-4 (B ends with one radix-2) steps over LDS images in which the transforms of a
// workgroup are interleaved (element i of transform f at i * batch + f), so that at every step consecutive threads read
// and write consecutive addresses.  Every twiddle is read from the one table of W_65536^k.

// (8-byte aligned: one LDS or memory access per element)
struct alignas(8) AnalysisComplex {
	float re, im;
};

GVTM_ANALYSIS_HD AnalysisComplex operator+(AnalysisComplex a, AnalysisComplex b) { return {a.re + b.re, a.im + b.im}; }
GVTM_ANALYSIS_HD AnalysisComplex operator-(AnalysisComplex a, AnalysisComplex b) { return {a.re - b.re, a.im - b.im}; }
GVTM_ANALYSIS_HD AnalysisComplex operator*(AnalysisComplex a, AnalysisComplex b)
{
	return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
// i (b): a quarter turn
GVTM_ANALYSIS_HD AnalysisComplex analysis_times_i(AnalysisComplex b) { return {-b.im, b.re}; }

// W_65536^e from the half table: W^(e + 32768) = -W^e
GVTM_ANALYSIS_HD AnalysisComplex analysis_twiddle(const AnalysisComplex* table, unsigned e)
{
	const AnalysisComplex w = table[e & (kAnalysisHalf - 1)];
	return (e & kAnalysisHalf) ? AnalysisComplex{-w.re, -w.im} : w;
}

// the LDS image of pass B keeps one element free behind every 32: its rows arrive along n1, 32 elements apart
struct AnalysisPlain {
	GVTM_ANALYSIS_HD static unsigned at(unsigned i) { return i; }
};
struct AnalysisPadded {
	GVTM_ANALYSIS_HD static unsigned at(unsigned i) { return i + (i >> 5); }
};

// Butterfly t of a radix-4 step on transforms of length n at stride s (n * s elements, n / 4 * s butterflies): the four
// results, twiddled, in y0 .. y3; they belong at q + s (4 p + l), which the caller stores (or sends to memory, at the last
// step, where p = 0 and q + s l is the element's final place).
template <typename Image>
GVTM_ANALYSIS_HD void analysis_radix4(const AnalysisComplex* x, unsigned n, unsigned s, unsigned t, const AnalysisComplex* table, AnalysisComplex y[4],
		unsigned& q, unsigned& p)
{
	const unsigned n1 = n / 4;
	q = t % s;
	p = t / s;
	const AnalysisComplex a = x[Image::at(q + s * p)], b = x[Image::at(q + s * (p + n1))];
	const AnalysisComplex c = x[Image::at(q + s * (p + 2 * n1))], d = x[Image::at(q + s * (p + 3 * n1))];
	const AnalysisComplex apc = a + c, amc = a - c, bpd = b + d, jbmd = analysis_times_i(b - d);
	const unsigned e = p * (kAnalysisSize / n); // W_n^p = W_65536^e
	y[0] = apc + bpd;
	y[1] = amc - jbmd;
	y[2] = apc - bpd;
	y[3] = amc + jbmd;
	// (also where p = 0 and the three are 1: a load that does not depend on a branch can be issued ahead of its use)
	y[1] = y[1] * analysis_twiddle(table, e);
	y[2] = y[2] * analysis_twiddle(table, 2 * e);
	y[3] = y[3] * analysis_twiddle(table, 3 * e);
}

template <typename Image>
GVTM_ANALYSIS_HD void analysis_radix4_step(const AnalysisComplex* x, AnalysisComplex* y, unsigned n, unsigned s, unsigned t, const AnalysisComplex* table)
{
	AnalysisComplex r[4];
	unsigned q, p;
	analysis_radix4<Image>(x, n, s, t, table, r, q, p);
	for (unsigned l = 0; l < 4; ++l) y[Image::at(q + s * (4 * p + l))] = r[l];
}

// pass A's input: element n of z for the buffer's samples (normalised, windowed; 0 behind the window).  Behind the window
// the loads go to element 0 and their result is dropped: loads that do not depend on a branch can be issued together.
// aligned8: one 8-byte load, where the buffer starts at an even sample of an aligned row.
template <bool aligned8>
GVTM_ANALYSIS_HD AnalysisComplex analysis_input(const float* s, float norm_coef, const double* window, unsigned W, unsigned n)
{
	const bool inside = 2 * n < W;
	const unsigned i = inside ? 2 * n : 0;
	float s0, s1;
	if constexpr (aligned8) {
		const AnalysisComplex pair = *reinterpret_cast<const AnalysisComplex*>(s + i);
		s0 = pair.re;
		s1 = pair.im;
	} else {
		s0 = s[i];
		s1 = s[i + 1];
	}
	const AnalysisComplex z = {analysis_windowed(analysis_normalised(s0, norm_coef), window[i]), analysis_windowed(analysis_normalised(s1, norm_coef), window[i + 1])};
	return inside ? z : AnalysisComplex{0.0f, 0.0f};
}

// the image's elements a thread loads, the butterflies of a radix-4 step it runs, and those of a radix-2 step: constant
// trip counts, so that the loops unroll and the memory loads of a whole loop are in flight together
constexpr unsigned kAnalysisLoads = 4096 / 256, kAnalysisButterflies4 = 1024 / 256, kAnalysisButterflies2 = 2048 / 256;

template <bool aligned8>
GVTM_ANALYSIS_HD void analysis_load_a(unsigned tid, unsigned g, const float* s, float norm_coef, const double* window, unsigned W, AnalysisComplex* u)
{
#pragma unroll 8
	for (unsigned j = 0; j < kAnalysisLoads; ++j) {
		const unsigned e = tid + j * 256, f = e % 16, n2 = e / 16;
		u[e] = analysis_input<aligned8>(s, norm_coef, window, W, (16 * g + f) + 128 * n2);
	}
}

constexpr unsigned kAnalysisThreads = 256;      // per workgroup of the passes A, B and C
constexpr unsigned kAnalysisN1 = 128, kAnalysisN2 = 256;
constexpr unsigned kAnalysisColumnsA = 16;      // columns n1 per workgroup of pass A: 16 x 256 elements
constexpr unsigned kAnalysisRowsB = 32;         // rows k2 per workgroup of pass B: 32 x 128 elements
constexpr unsigned kAnalysisImage = 4096;       // elements of either image
constexpr unsigned kAnalysisImagePadded = kAnalysisImage + kAnalysisImage / 32;
constexpr unsigned kAnalysisGroupsA = kAnalysisN1 / kAnalysisColumnsA, kAnalysisGroupsB = kAnalysisN2 / kAnalysisRowsB; // 8 and 8 per buffer

// Pass A, the work of thread tid of workgroup g (columns 16 g .. 16 g + 15) between two barriers: phase 0 loads, 1 to 3
// are the LDS steps (256 -> 64 -> 16 -> 4), 4 is the last step, whose results go to T twiddled.  u and v: the two images.
// (The phase is a template parameter so that every length and stride is a constant where it is used.)
template <int phase>
GVTM_ANALYSIS_HD void analysis_pass_a(unsigned tid, unsigned g, const float* s, float norm_coef, const double* window, unsigned W, bool aligned8,
		const AnalysisComplex* __restrict__ table, AnalysisComplex* u, AnalysisComplex* v, AnalysisComplex* __restrict__ T)
{
	constexpr unsigned B = kAnalysisColumnsA;
	static_assert(kAnalysisLoads * kAnalysisThreads == kAnalysisImage && B == 16 && kAnalysisN1 == 128, "analysis_load_a's numbers");
	if constexpr (phase == 0) {
		if (aligned8) analysis_load_a<true>(tid, g, s, norm_coef, window, W, u);
		else analysis_load_a<false>(tid, g, s, norm_coef, window, W, u);
	} else if constexpr (phase < 4) {
		const AnalysisComplex* x = (phase & 1) ? u : v;
		AnalysisComplex* y = (phase & 1) ? v : u;
		constexpr unsigned n = 1024u >> (2 * phase), st = B << (2 * (phase - 1)); // (256, 16), (64, 64), (16, 256)
#pragma unroll
		for (unsigned j = 0; j < kAnalysisButterflies4; ++j) analysis_radix4_step<AnalysisPlain>(x, y, n, st, tid + j * kAnalysisThreads, table);
	} else {
#pragma unroll
		for (unsigned j = 0; j < kAnalysisButterflies4; ++j) {
			const unsigned t = tid + j * kAnalysisThreads;
			AnalysisComplex r[4];
			unsigned q, p;
			analysis_radix4<AnalysisPlain>(v, 4, kAnalysisImage / 4, t, table, r, q, p);
			const unsigned n1 = B * g + q % B;
			for (unsigned l = 0; l < 4; ++l) {
				const unsigned k2 = q / B + (kAnalysisN2 / 4) * l;
				T[k2 * kAnalysisN1 + n1] = r[l] * analysis_twiddle(table, 2 * n1 * k2); // W_32768^(n1 k2)
			}
		}
	}
}

// Pass B, thread tid of workgroup h (rows 32 h .. 32 h + 31): phase 0 loads, 1 to 3 are the radix-4 steps (128 -> 32 -> 8
// -> 2), 4 the radix-2 step, whose results go to Z in natural order.
template <int phase>
GVTM_ANALYSIS_HD void analysis_pass_b(unsigned tid, unsigned h, const AnalysisComplex* __restrict__ T, const AnalysisComplex* __restrict__ table, AnalysisComplex* u,
		AnalysisComplex* v, AnalysisComplex* __restrict__ Z)
{
	constexpr unsigned B = kAnalysisRowsB;
	if constexpr (phase == 0) {
#pragma unroll 8
		for (unsigned j = 0; j < kAnalysisLoads; ++j) {
			const unsigned e = tid + j * kAnalysisThreads;
			const unsigned n1 = e % kAnalysisN1, r = e / kAnalysisN1;
			u[AnalysisPadded::at(n1 * B + r)] = T[(B * h + r) * kAnalysisN1 + n1];
		}
	} else if constexpr (phase < 4) {
		const AnalysisComplex* x = (phase & 1) ? u : v;
		AnalysisComplex* y = (phase & 1) ? v : u;
		constexpr unsigned n = 512u >> (2 * phase), st = B << (2 * (phase - 1)); // (128, 32), (32, 128), (8, 512)
#pragma unroll
		for (unsigned j = 0; j < kAnalysisButterflies4; ++j) analysis_radix4_step<AnalysisPadded>(x, y, n, st, tid + j * kAnalysisThreads, table);
	} else {
#pragma unroll
		for (unsigned j = 0; j < kAnalysisButterflies2; ++j) {
			const unsigned t = tid + j * kAnalysisThreads;
			const AnalysisComplex a = v[AnalysisPadded::at(t)], b = v[AnalysisPadded::at(t + kAnalysisImage / 2)];
			const unsigned k2 = B * h + t % B, k1 = t / B;
			Z[kAnalysisN2 * k1 + k2] = a + b;
			Z[kAnalysisN2 * (k1 + kAnalysisN1 / 2) + k2] = a - b;
		}
	}
}

// Pass C: bin k in [0, 32768] of the real transform from Z
GVTM_ANALYSIS_HD AnalysisComplex analysis_untangle(const AnalysisComplex* Z, const AnalysisComplex* table, unsigned k)
{
	const AnalysisComplex zk = Z[k & (kAnalysisHalf - 1)], zm = Z[(kAnalysisHalf - k) & (kAnalysisHalf - 1)];
	const AnalysisComplex even = {zk.re + zm.re, zk.im - zm.im}, odd = {zk.re - zm.re, zk.im + zm.im};
	const AnalysisComplex turned = analysis_twiddle(table, k) * odd;
	return {0.5f * (even.re + turned.im), 0.5f * (even.im - turned.re)};
}

GVTM_ANALYSIS_HD float analysis_magnitude(AnalysisComplex x)
{
	return sqrtf(x.re * x.re + x.im * x.im) * 0.00390625f;
}

#if defined(__HIP__)

// A batch on the device.  The pairs (utterance b, buffer k) are numbered b * max_buffers + k; a launch works on the pairs
// [first_pair, first_pair + n_pairs), pair j in slot j - first_pair of the scratch, and a pair behind its utterance's
// buffer count does nothing.  An utterance's count is taken as min(counts[b], audio_stride).
struct AnalysisArgs {
	const float* audio;
	size_t audio_stride;
	const int64_t* counts;      // [batch]
	const int64_t* first;       // [batch] or null
	size_t batch, max_buffers;
	size_t first_pair, n_pairs;
	unsigned W;
	unsigned n_bins;
	bool log_scale;
	float min_db;
	const double* window;            // [W]
	const AnalysisComplex* table;    // [32768]
	float* norm_coefs;               // [n_pairs] scratch
	AnalysisComplex* T;              // [n_pairs][32768] scratch
	AnalysisComplex* Z;              // [n_pairs][32768] scratch
	float* spectra;                  // [batch][max_buffers][n_bins] or null
	float* signal;                   // [batch][max_buffers][W] or null
	int32_t* buffers_out;            // [batch] or null (written by the launch whose first_pair is 0)
	// null: the outputs' row of pair (b, k) is the pair's number, b * max_buffers + k.  Else utterance b's buffers go to the
	// rows out_slots[b] + k of its block of out_stride rows (a listening stream's queues: vtm_listen.hpp)
	const int32_t* out_slots;        // [batch] or null
	size_t out_stride;
};

// the kernels of one slice on `stream`: counts (first slice only), peak + signal view, and with spectra the passes A, B, C
hipError_t launch_analysis(const AnalysisArgs& args, hipStream_t stream);

#endif

} // namespace gvtm
