// Launch interface between the C ABI (vtm_capi_*.cpp, vtm_host.hpp) and the kernels (vtm_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "vtm_design.hpp"
#include "vtm_targets.hpp" // (the walk of the synthesis kernel's targets driver: vtm_kernel_v2.inc is included inside a namespace)

namespace gvtm {

// ---- streams (gvtm_stream_*): what an utterance carries from one launch to the next, in device memory ----
//
//   StreamHeader | scalars CT[kStreamScalars] | tube CT[lanes][2 * SectionDelay + 1] | decimator pre-roll CT[48] | ring ST[xr]
//   | targets sums double[16]
//
// i.e. exactly the reference model's members that survive a step (vtm/VocalTractModel0.h:221-252): the section delay
// lines, the filter memories, the oscillator phase, the noise seed, the decimator's and the converter's buffers with
// the converter's position (time register and pointers follow from the number of steps, SampleRateConverter.h:268-282).
// A fresh utterance (create / reset) is all zeros except the noise seed (NoiseSource.h:32-34).
struct StreamHeader {
	unsigned long long step_base; // internal steps synthesized so far
	double seed;                  // NoiseSource::seed_
	unsigned peak_bits;           // running max |sample| as float bits
	unsigned reserved_;
	unsigned long long pad_;
};
static_assert(sizeof(StreamHeader) == 32, "stream header layout");
constexpr int kStreamScalars = 12;
constexpr int kSsPos = 0, kSsPrev = 1;           // oscillator position, previous white-noise sample
constexpr int kSsBp = 2, kSsThr = 6;             // band-pass x1 x2 y1 y2, throat y1
constexpr int kSsRadMouth = 7, kSsRadNose = 9;   // radiation filters {x1, y1}
constexpr int kStreamPreRoll = 48;               // = kWPre of the kernel
enum StreamMode : int { kStreamNone = 0, kStreamPush = 1, kStreamFinish = 2 };

template <typename CT, typename ST>
struct StreamLayout {
	static constexpr size_t scalars() { return sizeof(StreamHeader); }
	static constexpr size_t tube() { return scalars() + sizeof(CT) * kStreamScalars; }
	static constexpr size_t wpre(int lanes, int words) { return tube() + sizeof(CT) * static_cast<size_t>(lanes) * words; }
	static constexpr size_t ring(int lanes, int words) { return wpre(lanes, words) + sizeof(CT) * kStreamPreRoll; }
	// behind the ring (no other offset moves): the 16 sums of a targets-fed run's moving averages (vtm_targets.hpp), doubles
	// whatever CT is -- the one state of the interpolation wavefront, which a run fed frames does not have
	static constexpr size_t sums(int lanes, int words, int xr) { return (ring(lanes, words) + sizeof(ST) * static_cast<size_t>(xr) + 7) & ~size_t(7); }
	static constexpr size_t bytes(int lanes, int words, int xr) { return (sums(lanes, words, xr) + sizeof(double) * GVTM_N_PARAM + 15) & ~size_t(15); }
};

// Reference model 5 (VocalTractModel5, vtm/VocalTractModel5.h:523-579): what its members keep between steps -- the scans'
// phases, noise seed and low-pass memories, the recursive filter halves' memories, the last inputs of their feed-forward
// halves, every section's top / bottom flow and radiation-impedance memories, the converter's 1024-sample ring and the
// ring of converted samples the difference filter looks back into.  A fresh utterance is zeros except the Rosenberg
// source's t2 (RosenbergBGlottalSource::reset) and the noise seed.
constexpr int kS5Scan = 0;     // t, t2, seed, glottal-noise x1 y1, frication-noise x1 x2 y1 y2
constexpr int kS5Gp = 9;       // glottal low-pass y1
constexpr int kS5Bp = 10;      // band-pass y1, y2
constexpr int kS5Fo = 12;      // transmitted flow y1: mouth, nose
constexpr int kS5ValLast = 14; // last pulse value (the low-pass's x1)
constexpr int kS5FnmLast = 15; // last two band-pass inputs (x2, x1)
constexpr int kS5Carry = 17;   // last flow into mouth, nose
constexpr int kStream5Scalars = 24;
struct Stream5Layout {
	static constexpr size_t scalars() { return sizeof(StreamHeader); }
	static constexpr size_t tube() { return scalars() + sizeof(double) * kStream5Scalars; }
	static constexpr size_t ring() { return tube() + sizeof(double) * 51 * 4; }
	static constexpr size_t yring() { return ring() + sizeof(double) * kSrcRing; }
	// behind the ring of converted samples (no other offset moves): the 16 sums of a targets-fed run's moving averages
	// (vtm_targets.hpp), doubles in both classes -- only 5 of the 24 scalar slots are free.  Every model 5 stream has them; a
	// run fed frames never touches them
	static constexpr size_t sums() { return (yring() + sizeof(float) * 512 + 7) & ~size_t(7); }
	static constexpr size_t bytes() { return (sums() + sizeof(double) * GVTM_N_PARAM + 15) & ~size_t(15); }
};
static_assert(Stream5Layout::sums() == 12096 && Stream5Layout::bytes() == 12224, "model 5 stream state layout");

// Plan constants of the all-float kernel as floats, by value behind the 64 coefficient slots of SynthArgs::fir_k: the
// helper passes and the filter wavefronts then take them from scalar registers instead of reading DeviceConstants' doubles
// in LDS and converting them per lane and pass.  A float plan's constants are floats widened, so these are the same numbers.
enum FloatConst : int {
	kKfRadiusCoef = 0, // [8]
	kKfAperture2 = 8, kKfNasalR2Sq, kKfBasicIncrement, kKfBpT, kKfBreathiness, kKfCrossmix, kKfThroatB0, kKfThroatA1, kKfThroatGain,
	kKfMouthARad, kKfNoseARad, kKfNasalK5, kKfCount
};
constexpr int kFirKConsts = 64; // SynthArgs::fir_k.f[kFirKConsts + FloatConst]

struct SynthArgs {
	DeviceConstants k;              // by value (host-side launch decisions)
	const DeviceConstants* kconst;  // the same constants in device memory (the kernel stages them in LDS)
	const float* params;         // [batch][max_frames][16]
	const int32_t* frame_counts; // [batch] or null
	float* audio;                // [batch][audio_stride]
	int64_t* out_counts;         // [batch] or null
	float* maxabs;               // [batch] or null
	const void* wavetable;       // [512]      design tables: double, or float for GVTM_PRECISION_F32
	const void* fir;             // [fir_taps]
	// by value, read with scalar loads: f[kFirKConsts + FloatConst] holds the float kernel's plan constants (above), f[0..47)
	// the float design's coefficients.  The float decimator's unrolled tap loop takes its coefficients as the literals of
	// kGlottalFirF32 (fir_literals below); only the two float shapes that measured slower that way read f[0..47), from SGPRs
	// (vtm_kernel_v2.inc: fir_literal_taps).  The double and mixed kernels read `fir` through LDS.  (d is unused: it keeps
	// the block's size and alignment, and with them the layout of the arguments behind it.)
	union FirByValue { double d[49]; float f[98]; } fir_k;
	static_assert(sizeof(FirByValue) == sizeof(double) * 49 && kFirKConsts + kKfCount <= 98, "float constants fit behind the float coefficients");
	const void* src_h;           // [3328]
	const void* src_dh;          // [3328]
	const void* noise_lp = nullptr;  // [noise_len] the noise source's low-passed samples by internal step (one-shot launches), or
	                                 // null: the scan wavefront generates them (streams, whose step count has no bound)
	unsigned long long noise_len = 0;
	size_t max_frames;
	size_t audio_stride;
	size_t batch;
	int xr;                      // internal-rate ring length per utterance (a power of two; synth_launch_shape())
	unsigned char* stream = nullptr; // null, or [batch] stream states of stream_stride bytes each (layout above)
	size_t stream_stride = 0;
	int stream_mode = kStreamNone;   // StreamMode
	double* debug_taps;          // null, or [batch][max_frames*control_steps][8] per-step taps (tests only)
	unsigned long long* phase_cycles; // null, or [workgroups][16] shader cycles per role wavefront and helper stage (diagnostics only)
	const Model5Constants* k5const = nullptr; // model 5 only: its constants in device memory
	// launches of several voices (set: launch_synth / launch_synth5 run the voice variant): kconst and wavetable (model 5:
	// kconst and k5const) then hold one block per voice
	const int32_t* row_map = nullptr;     // [groups][rows] utterance of each workgroup row, -1 = none
	const int32_t* group_voice = nullptr; // [groups] voice of each workgroup, -1 = none (the workgroup exits)
	// several voices in a stream (v2 kernel): the chunk that fixes each voice's ring, synth_ring_for(its upsampling, its
	// pad, stream_chunk) -- the one-row shape's, so that every launch shape keeps the ring a single-voice stream of that
	// voice has
	int stream_chunk = 0;
	// float plans: `fir` is kGlottalFirF32 bit for bit (the plan compared them when it was made), so the decimator's
	// unrolled tap loop runs, with its coefficients from that table as literals; 0: the generic loop over `fir`
	int fir_literals = 0;
	// float plans that up-sample: the converter's coefficients by output phase, [src_phase_mask + 1][kSrcPhaseRecord] floats
	// in device memory (vtm_design.hpp: design_src_phase_table; the plan uploads it once), read by the shapes
	// v2::src_phase_table() names; null: every shape forms the coefficients from the LDS table, pass by pass
	const float* src_phase = nullptr;
	unsigned src_phase_mask = 0;
	// the voice's wavetable never follows the amplitude (vtm_design.hpp: static_wavetable): the shapes
	// v2::static_wavetable_pass() names look the two entries up and read neither amplitude nor constants; 0: wavetable_entry
	int static_wavetable = 0;
	// launches from parameter targets (tg_offsets set: launch_synth runs the targets variant, vtm_kernels_targets.hip; the
	// kernel's kTargetsFlag): utterance b's parameter p walks list l = tg_ids ? tg_ids[16 b + p] : 16 b + p, the points
	// [tg_offsets[l], tg_offsets[l + 1]) of tg_steps / tg_values, through a moving average of tg_N samples (vtm_targets.hpp).
	// frame_counts then holds the utterances' STEP counts (never null: the check kernel's, 0 for a refused utterance),
	// max_frames the most steps of an utterance, and params is unused
	const int64_t* tg_offsets = nullptr;
	const int32_t* tg_ids = nullptr;
	const int32_t* tg_steps = nullptr;
	const float* tg_values = nullptr;
	int64_t tg_N = 0;
	double tg_invN = 0.0;
	// targets under several voices (row_map and tg_offsets set: vtm_kernels_targets_voices.hip): the filter's length and its
	// reciprocal by voice, [n_voices] each in device memory (the plan uploads them once); tg_N and tg_invN are then unused
	const int64_t* tg_voice_N = nullptr;
	const double* tg_voice_invN = nullptr;
};

struct GroupVoicesArgs {
	const int32_t* voice_ids; // [batch]
	size_t batch;
	int n_voices;
	int rows;                 // utterances per workgroup
	size_t groups;            // ceil(batch / rows) + n_voices: what any mix of ids needs
	int32_t* row_map;         // [groups][rows] out
	int32_t* group_voice;     // [groups] out
	int32_t* counts;          // [n_voices][kGroupVoicesThreads] scratch
	int64_t* out_counts;      // [batch] or null: -1 for an id outside [0, n_voices)
	float* maxabs;            // [batch] or null: 0 for such an id
};
constexpr int kGroupVoicesThreads = 256;

struct NormalizeArgs {
	const float* audio;
	const int64_t* counts; // or null
	const float* maxabs;
	float* out_f32;        // or null
	int16_t* out_i16;      // or null
	float* scales;         // or null
	size_t audio_stride;
};

// The shape of one synthesis launch: utterances per workgroup (1, 2, 4 or 8; model 5: 1 or 2), samples of an utterance's
// internal-rate ring (model 5: 0, its ring is a constant of its kernel), LDS bytes per workgroup.  rows == 0: none fits.
struct LaunchShape {
	int rows = 0;
	int ring = 0;
	size_t lds = 0;
	int forced = 0; // what names this shape again as synth_launch_shape's forced_rows: the rows; model 5 (either class): 1 + its shape's index
	int per_cu = 0; // utterances one compute unit holds in this shape: rows x the workgroups it holds at once (model 5's float class: up to 2)
};
constexpr size_t kLdsPerWorkgroup = 160 * 1024;
// THE row choice, for every caller.  voices: the plan's designs (voices[0] says whether model 5); forced_rows: 1, 2, 4 or 8
// names the rows (model 5: 1 or 2 name the shape of index 0 or 1 of its class, vtm_kernel_m5.inc: two utterances per
// workgroup in the double class, the chunk of 56 steps in the float class), anything else leaves them to `batch`;
// several_voices: the kernel's voice variant (at most 4 rows, model 5: 1); stream_ring: a stream's fixed ring, or 0 for the longest own ring of the voices (the reference's
// BUFFER_SIZE (1024) when down-sampling, so that the flush overrun aliases as the reference's ring does; otherwise the
// smallest power of two holding two chunks, the resampler's history and the flush zeros).  With `fit`, rows whose LDS
// exceeds kLdsPerWorkgroup give way to half as many (not model 5) or to "none fits"; without, they stay whatever their LDS.
// targets: a launch from parameter targets; it changes the answer for model 5 alone, whose targets variant has shapes of its
// own by the same index (vtm_kernel_m5.inc: m5_targets_shape; with several_voices its one-utterance shapes).
LaunchShape synth_launch_shape(const Design* voices, int n_voices, int precision, size_t batch, int forced_rows, bool several_voices,
		int stream_ring = 0, bool fit = true, bool targets = false);// the chunk length (internal steps per tick) of a shape, which its own ring length follows; 0: no such shape
int synth_chunk_length(const DeviceConstants& k, int precision, int rows);
// which of its serial filter stages a single-voice shape runs with the feed-forward half 64 steps at a time
// (v2::filter_split_f2: bit 0, the post-tube filters); 0: none, or no such shape
int synth_filter_split(const DeviceConstants& k, int precision, int rows);
// batch: utterances, or with args.row_map set (several voices) the workgroups of launch_group_voices' map, of one voice
// each (args.xr: the longest ring of the voices; a stream's rings follow args.stream_chunk)
hipError_t launch_synth(const SynthArgs& args, size_t batch, int precision, int rows, hipStream_t stream);
// the targets variant alone (vtm_kernels_targets.hip; launch_synth calls it where args.tg_offsets is set): one voice, one,
// two or four rows
hipError_t launch_synth_targets(const SynthArgs& args, size_t batch, int precision, int rows, hipStream_t stream);
// the targets variant of several voices alone (vtm_kernels_targets_voices.hip; launch_synth calls it where args.tg_offsets
// and args.row_map are set): `groups` workgroups of launch_group_voices' map, one, two or four rows
hipError_t launch_synth_targets_voices(const SynthArgs& args, size_t groups, int precision, int rows, hipStream_t stream);
// bytes of one utterance's stream state for a plan (ring length of the one-row shape: streams whose utterances are not in
// lockstep run one utterance per workgroup, and every shape of a stream uses that ring length)
size_t stream_state_bytes(const DeviceConstants& k, int precision, int xr);
// several voices: builds args.row_map / args.group_voice from the voice ids (one small workgroup, stable counting sort)
hipError_t launch_group_voices(const GroupVoicesArgs& args, hipStream_t stream);
// reference model 5: VocalTractModel5<double,1> (GVTM_PRECISION_F64) or VocalTractModel5<float,1> (GVTM_PRECISION_F32) in
// the shape `index` (0 or 1: LaunchShape::forced - 1) of that class; with args.row_map set (several voices: one constants
// block of each kind per voice) the double class's index 0 only or either index of the float class, and `batch` is the
// number of workgroups.
hipError_t launch_synth5(const SynthArgs& args, size_t batch, int precision, int index, hipStream_t stream);
// the float class alone (vtm_kernels_m5f.hip; launch_synth5 calls it), and the LDS bytes of a workgroup of its shape `index`
hipError_t launch_synth5_float(const SynthArgs& args, size_t batch, int index, hipStream_t stream);
size_t synth5_float_lds_bytes(int index);
// the voice variant alone (vtm_kernels_m5v.hip; launch_synth5 calls it): `groups` workgroups of one utterance each
hipError_t launch_synth5_voices(const SynthArgs& args, size_t groups, hipStream_t stream);
// the voice variant of the float class alone (vtm_kernels_m5fv.hip; launch_synth5 calls it), in the float class's shape `index`
hipError_t launch_synth5_float_voices(const SynthArgs& args, size_t groups, int index, hipStream_t stream);
// the targets variants alone (vtm_kernels_m5t.hip: the double class; vtm_kernels_m5ft.hip: the float class; launch_synth5
// calls them where args.tg_offsets is set and args.row_map is not), in the shape `index` of the class's targets shapes (m5_targets_shape): one voice,
// one-shot launches and a stream's (args.stream: the points are the stream's log, in absolute steps)
hipError_t launch_synth5_targets(const SynthArgs& args, size_t batch, int index, hipStream_t stream);
hipError_t launch_synth5_float_targets(const SynthArgs& args, size_t batch, int index, hipStream_t stream);
// what both ask of their arguments: the lists, the steps in frame_counts, the filter's length; no row map
inline bool synth5_targets_args(const SynthArgs& args)
{
	return args.k5const && args.tg_offsets && args.tg_steps && args.tg_values && args.frame_counts && args.tg_N >= 1 && !args.row_map;
}
// the targets variants under several voices alone (vtm_kernels_m5tv.hip: the double class, its one-utterance shape;
// vtm_kernels_m5ftv.hip: the float class, in its targets shape `index`; launch_synth5 calls them where args.tg_offsets and
// args.row_map are both set): `groups` workgroups of launch_group_voices' map, one utterance each, one-shot launches and a
// stream's (args.stream: the points are the stream's log, in absolute steps, and every state address follows the row map)
hipError_t launch_synth5_targets_voices(const SynthArgs& args, size_t groups, hipStream_t stream);
hipError_t launch_synth5_float_targets_voices(const SynthArgs& args, size_t groups, int index, hipStream_t stream);
// what both ask of their arguments: the row map and the groups' voices, the lists, the steps in frame_counts, the filter's
// length and reciprocal by voice
inline bool synth5_targets_voices_args(const SynthArgs& args)
{
	return args.k5const && args.row_map && args.group_voice && args.tg_offsets && args.tg_steps && args.tg_values && args.frame_counts && args.tg_voice_N &&
	       args.tg_voice_invN;
}
constexpr int kDppSelftestInts = 640;
hipError_t launch_dpp_selftest(int* d_out /* [kDppSelftestInts] */, hipStream_t stream);
hipError_t launch_float_math_probe(int kind, const float* d_x, size_t n, float* d_out, hipStream_t stream);
hipError_t launch_normalize(const NormalizeArgs& args, size_t batch, hipStream_t stream);

} // namespace gvtm
