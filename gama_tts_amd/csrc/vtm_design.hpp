// Host-side design of everything that is fixed for a voice configuration:
// derived rates, filter constants and the fp64 tables the device kernels stage
// in LDS.  All of it is computed in fp64 on the host exactly once per plan
// (design tables must be fp64 even for the mixed-precision path).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gama_vtm.h"

namespace gvtm {

constexpr int kWavetableLength = 512;   // WavetableGlottalSource.h:91
constexpr int kSrcZeroCrossings = 13;   // SampleRateConverter.h:49
constexpr int kSrcPhases = 256;         // L_RANGE, SampleRateConverter.h:46
constexpr int kSrcFilterLength = kSrcZeroCrossings * kSrcPhases; // 3328
constexpr int kSrcRing = 1024;          // BUFFER_SIZE, SampleRateConverter.h:44
constexpr int kMaxFirTaps = 64;
constexpr int kMaxSectionDelay = 4;
constexpr int kMaxPad = 96;

// The 2:1 decimator of the glottal source as designed in float: design_glottal_fir<float>() (vtm_design.cpp) takes no
// argument -- WavetableGlottalSourceFIRFilter::maximallyFlat with the three constants of WavetableGlottalSource.h:94-96 --
// so these 47 coefficients are the same for every voice, rate and plan.  Host and device share them: the float kernels
// take them as 32-bit literals, and a plan compares its own design with them bit for bit before it says so
// (vtm_capi_plan.cpp; SynthArgs::fir_literals).  Made from this project's own design: the values design_glottal_fir<float>()
// returns (a float plan's gvtm_plan_table(GVTM_TABLE_FIR)), each printed exactly as a hexadecimal float;
// tests/test_fir_literals_cpu.py holds the two against each other.
constexpr int kGlottalFirTapsF32 = 47;
constexpr float kGlottalFirF32[kGlottalFirTapsF32] = {
	0x1.7104f6p-24f, 0x1.e9efcap-23f, -0x1.a0e112p-25f, -0x1.45ce18p-19f,
	-0x1.a55396p-18f, 0x1.2af00ap-19f, 0x1.6ac7fap-15f, 0x1.246622p-14f,
	-0x1.6c9652p-14f, -0x1.c5647cp-12f, -0x1.2c53bp-12f, 0x1.28a494p-10f,
	0x1.3159f6p-9f, -0x1.43030ep-11f, -0x1.d0b9fp-8f, -0x1.842804p-8f,
	0x1.6f26b8p-7f, 0x1.9513bp-6f, -0x1.6560f2p-10f, -0x1.cb1d68p-5f,
	-0x1.a3d234p-5f, 0x1.67d89cp-4f, 0x1.2f9eccp-2f, 0x1.9809a4p-2f,
	0x1.2f9eccp-2f, 0x1.67d89cp-4f, -0x1.a3d234p-5f, -0x1.cb1d68p-5f,
	-0x1.6560f2p-10f, 0x1.9513bp-6f, 0x1.6f26b8p-7f, -0x1.842804p-8f,
	-0x1.d0b9fp-8f, -0x1.43030ep-11f, 0x1.3159f6p-9f, 0x1.28a494p-10f,
	-0x1.2c53bp-12f, -0x1.c5647cp-12f, -0x1.6c9652p-14f, 0x1.246622p-14f,
	0x1.6ac7fap-15f, 0x1.2af00ap-19f, -0x1.a55396p-18f, -0x1.45ce18p-19f,
	-0x1.a0e112p-25f, 0x1.e9efcap-23f, 0x1.7104f6p-24f,
};

// Everything the kernels need besides the tables; plain data, copied to the device by value.
struct DeviceConstants {
	// rates and driver loop
	int sample_rate;          // internal rate
	unsigned control_steps;   // steps per frame
	float interp_coef;        // 1.0f / control_steps (float32, Controller.cpp:287)
	int section_delay;
	int layout;               // gvtm_tube_layout
	// sources
	int waveform;             // 0 pulse, 1 sine
	int modulation;
	unsigned table_div1, table_div2;
	double tn_delta;          // 0 => static wavetable
	double basic_increment;   // 512 / fs
	double breathiness;       // breathiness / 100
	double crossmix_factor;   // 1 / amp60(mix_offset)
	int fir_taps;
	// tube
	double damping;
	double radius_coef[8];
	double aperture_radius2;  // apertureRadius^2
	double nasal_r2_sq;       // nasalRadius[N2]^2 (first nasal junction)
	double nasal_k[6];        // fixed nasal coefficients; [0] unused (time varying)
	double mouth_b0_refl, mouth_a1_refl, mouth_a_rad; // ReflectionFilter / RadiationFilter constants
	double nose_b0_refl, nose_a1_refl, nose_a_rad;
	double throat_b0, throat_a1, throat_gain;
	double bp_T;              // 1 / fs for BandpassFilter::update
	// sample-rate converter
	int upsampling;
	int pad;
	unsigned time_inc;        // timeRegisterIncrement_
	unsigned phase_inc;       // phaseIncrement_ (down-sampling)
	double src_ratio;         // sampleRateRatio_
};

// VocalTractModel5 only: what initializeSynthesizer (vtm/VocalTractModel5.h:455-521) derives besides the numbers
// shared with the other models (rates, driver loop, radius coefficients, damping, resampler in DeviceConstants)
struct Model5Constants {
	double sample_rate;        // sampleRate_ (TFloat, not truncated)
	double output_rate;
	int bypass, constant_mouth;
	double rb_t1, rb_tn_min, rb_tn_max;      // RosenbergBGlottalSource (vtm/RosenbergBGlottalSource.h:66-96)
	double gn_b0, gn_a1;                     // glottal-noise Butterworth1 (vtm/Butterworth1LowpassFilter.h:63-76)
	double gp_b0, gp_a1;                     // glottal-pulse Butterworth1
	double fn_b0, fn_b1, fn_a1, fn_a2;       // frication-noise Butterworth2 (vtm/Butterworth2LowpassFilter.h:88-107)
	double frication_factor;
	double min_loss, max_loss;               // min/max_glottal_loss / 100
	double nasal_r1_sq;                      // nasalRadius[NR2]^2: right side of the first nasal junction
	double nasal_k[6];                       // [1..5]: fixed nasal junctions NJ2..NJ6; [0] unused (time varying)
	double period;                           // PoleZeroRadiationImpedance::samplePeriod_
	double nose_c[6];                        // cT1, cT2, cT3, cR1, cR2, cR3 at the nose (fixed radius)
	double mouth_c[6];                       // the same at the mouth when its radius is constant
};

struct Design {
	bool model5 = false;
	gvtm5_config config5{};
	Model5Constants k5{};
	gvtm_config config;
	double control_rate;
	DeviceConstants k;
	std::vector<double> fir;        // fir_taps
	std::vector<double> src_h;      // 3328
	std::vector<double> src_dh;     // 3328
	std::vector<double> wavetable;  // 512
	// GVTM_PRECISION_F32: the tables as designed in float (the double vectors above hold the same values widened)
	bool f32 = false;
	std::vector<float> fir_f, src_h_f, src_dh_f, wavetable_f;
};

// The noise source's low-passed samples for internal steps [0, n) (NoiseSource.h:40-44 with its fixed seed,
// NoiseFilter.h:63-68): every utterance of every batch draws the same sequence after reset(), so a plan tabulates it
// once; `out` holds n floats (as_float: the sum formed in float as NoiseFilter<float> does) or n doubles.
void design_noise_table(size_t n, bool as_float, void* out);

// The up-sampling converter's polyphase coefficients by output phase, for a float plan of the models 0 to 4.
//
// Output sample ko reads the filter at frac = (ko * time_inc) & 0xFFFF (SampleRateConverter.h:330-372), so its 26
// coefficients h + dh * (m / 256) are a function of ko mod P alone, P = 2^16 / gcd(time_inc, 2^16) -- a power of two.
// A record is kSrcPhaseRecord floats: the 13 coefficients of the first wing (l = frac >> 8, m = frac & 255, entries
// l + 256 j), the 13 of the second (the same of ~frac), in the order the wings consume them, and two zeros that make a
// record seven 16-byte loads from one address.  Each coefficient is made with the float operations of the kernel's
// mad(dh, m / 256, h) on the plan's own float tables: the product rounded on its own, then the add (vtm_design.cpp is
// compiled without FMA contraction).
// Plans beyond kSrcPhaseCap phases have none (16384 records are 1.8 MB, under half of an XCD's 4 MB of L2; the next
// power of two would fill it), nor have down-sampling plans, whose phase walk has no fixed set of 26 entries.
constexpr int kSrcPhaseRecord = 28;
constexpr unsigned kSrcPhaseCap = 16384;
// P for a plan that takes the table, 0 for one that does not
unsigned src_phase_count(const Design& d);
// [src_phase_count(d)][kSrcPhaseRecord] floats (empty where the count is 0)
std::vector<float> design_src_phase_table(const Design& d);
// a voice whose glottal wavetable never follows the amplitude (tn_min == tn_max, or the sine: the first test of the
// kernels' wavetable_entry, decided once)
inline bool static_wavetable(const DeviceConstants& k) { return k.tn_delta == 0.0 || k.waveform != 0; }

// Returns "" on success, otherwise a description of the offending value.
std::string design_plan(const gvtm_config& cfg, double control_rate, Design& out);

std::string design_plan5(const gvtm5_config& cfg, double control_rate, Design& out);
// VocalTractModel5<float,1>: cfg.precision must be GVTM_PRECISION_F32; out.f32 is set, the constants are floats widened
std::string design_plan5_float(const gvtm5_config& cfg, double control_rate, Design& out);

// PoleZeroRadiationImpedance::update (vtm/PoleZeroRadiationImpedance.h:139-177): radius in metres -> cT1..3, cR1..3
void radiation_impedance(double radius, double period, double out[6]);

// Util::amplitude60dB (vtm/VTMUtil.h:48-67)
double amplitude_60db(double db);

#if defined(__HIPCC__)
#define GVTM_DESIGN_HD __host__ __device__ inline
#else
#define GVTM_DESIGN_HD inline
#endif

// Output bookkeeping of SampleRateConverter for a track of `steps` internal samples (host and device).
//
// Output sample k is emitted while its integer read position P_k = floor(k * time_inc / 2^16) lies before the end
// pointer; the final end pointer (after flushBuffer()'s 2 * pad zero fills, SampleRateConverter.h:462-471) is
// fills = steps + 2 * pad, so normally N = ceil(fills * 2^16 / time_inc) = k_from.
//
// The flush overrun (SampleRateConverter.h:298-308): when down-sampling the read position advances by more than one
// input per output, so an automatic dataEmpty() (every fill_size = 1024 - 2 * pad fills) can leave the empty pointer
// BEYOND its end pointer.  If fewer fills than that overshoot follow before flushBuffer()'s explicit dataEmpty(), it
// finds endPtr < emptyPtr_, adds BUFFER_SIZE and converts one more lap of the ring: outputs [k_from, k_to) with read
// positions up to fills + 1024, taken from the ring's leftovers.  Returns whether that happens.
// internal-rate ring of a workgroup row for a chunk of `chunk` steps: a power of two holding two chunks, the resampler's
// history and the flush zeros (+ 64: the resampler emits on a 64-aligned grid of outputs, so up to 63 outputs = at most
// 64 inputs wait a chunk longer); the reference's own BUFFER_SIZE when down-sampling (the flush overrun reads the ring's
// leftovers modulo that length, vtm_kernel_v2.inc's epilogue).  The host sizes launches with it, and a launch of several
// voices computes each workgroup's own from its voice's constants.
GVTM_DESIGN_HD int synth_ring_for(int upsampling, int pad, int chunk)
{
	if (!upsampling) return kSrcRing;
	int xr = 128;
	while (xr < 2 * chunk + 4 * pad + 64) xr *= 2;
	return xr;
}

GVTM_DESIGN_HD bool src_flush_overrun(unsigned time_inc, int pad, uint64_t steps, uint64_t& k_from, uint64_t& k_to)
{
	const uint64_t fills = steps + 2ull * static_cast<uint64_t>(pad);
	const uint64_t fill_size = static_cast<uint64_t>(kSrcRing - 2 * pad);
	const uint64_t last_auto_end = (fills / fill_size) * fill_size; // end pointer of the last automatic dataEmpty()
	k_from = ((fills << 16) + time_inc - 1) / time_inc;
	k_to = k_from;
	if (last_auto_end == 0) return false;
	const uint64_t k_star = ((last_auto_end << 16) + time_inc - 1) / time_inc; // first output it did not emit
	const uint64_t p_star = (k_star * static_cast<uint64_t>(time_inc)) >> 16; // where it left the empty pointer
	if (p_star <= fills) return false;
	k_to = (((fills + static_cast<uint64_t>(kSrcRing)) << 16) + time_inc - 1) / time_inc;
	return true;
}

// samples in outputBuffer() after finishSynthesis()
GVTM_DESIGN_HD uint64_t src_output_count(unsigned time_inc, int pad, int upsampling, uint64_t steps)
{
	uint64_t k_from = 0, k_to = 0;
	if (upsampling) return (((steps + 2ull * static_cast<uint64_t>(pad)) << 16) + time_inc - 1) / time_inc;
	return src_flush_overrun(time_inc, pad, steps, k_from, k_to) ? k_to : k_from;
}

// The output sample ranges of a launch's chunks without a division per chunk (host, device and
// tests/test_bounds_recurrence_cpu.py run this text).
//
// The first output sample whose read position lies at or behind internal sample n is Q(n) = ceil(n * 2^16 / time_inc),
// here as q = (n * 2^16 + time_inc - 1) / time_inc with its remainder r.  A chunk of C steps further on the numerator has
// grown by C * 2^16 = dq * time_inc + dr, so q grows by dq and r by dr, with one carry into q when r reaches time_inc:
// integers throughout, hence exactly the value the division gives.  The kernels that go this way divide twice per
// utterance and launch (the quotient at step_base, which is Extent::k_first and whose remainder one multiplication gives,
// and the end of the last chunk, which is no multiple of C away) and advance once per chunk.
struct SrcBounds {
	unsigned long long q; // (n * 2^16 + time_inc - 1) / time_inc
	unsigned r;           // (n * 2^16 + time_inc - 1) % time_inc
};
struct SrcBoundsStep {
	unsigned dq, dr; // (C * 2^16) / time_inc and % time_inc (dq is 0 when down-sampling by more than C)
};

GVTM_DESIGN_HD SrcBoundsStep src_bounds_step(unsigned time_inc, int chunk)
{
	const unsigned span = static_cast<unsigned>(chunk) << 16; // (a chunk is at most a few hundred steps)
	return SrcBoundsStep{span / time_inc, span % time_inc};
}

GVTM_DESIGN_HD SrcBounds src_bounds_at(unsigned time_inc, uint64_t n)
{
	const uint64_t x = (n << 16) + time_inc - 1;
	const uint64_t q = x / time_inc;
	return SrcBounds{q, static_cast<unsigned>(x - q * time_inc)};
}

// from internal sample n to n + C
GVTM_DESIGN_HD void src_bounds_advance(SrcBounds& b, SrcBoundsStep s, unsigned time_inc)
{
	// r + dr >= time_inc, asked without forming a sum that may not fit 32 bits (dr < time_inc)
	const bool carry = b.r >= time_inc - s.dr;
	b.q += static_cast<unsigned long long>(s.dq) + (carry ? 1u : 0u);
	b.r = carry ? b.r - (time_inc - s.dr) : b.r + s.dr;
}

// the largest src_output_count() over all tracks of at most `steps` internal samples: what a row of a ragged batch
// must be able to hold (a shorter track that runs into the flush overrun can be LONGER than the longest track)
inline uint64_t src_output_capacity(unsigned time_inc, int pad, int upsampling, uint64_t steps)
{
	const uint64_t lap = upsampling ? 0ull : static_cast<uint64_t>(kSrcRing);
	return (((steps + 2ull * static_cast<uint64_t>(pad) + lap) << 16) + time_inc - 1) / time_inc;
}

// --- parameter-track generation (vtm_tracks.hip) ---

// gvtm_track_config with the drift generator's filter designed (DriftGenerator::setUp,
// Butterworth2LowPassFilter<double>::update) — plain data, passed to the kernel by value
struct TrackConstants {
	int control_period;
	int macro_intonation, micro_intonation, intonation_drift, smooth_intonation;
	double initial_pitch, mean_pitch;
	double pitch_deviation, pitch_offset; // deviation * 2, deviation
	double b0, b1, a1, a2;                // Butterworth2LowPassFilter coefficients
};

// "" on success, otherwise what is wrong with the configuration
const char* design_tracks(const gvtm_track_config& cfg, TrackConstants& out);

// frames generateOutput() pushes for one event list (host; the loop over control periods without the arithmetic)
size_t tracks_frame_count(int control_period, const gvtm_event* events, size_t n_events);

} // namespace gvtm
