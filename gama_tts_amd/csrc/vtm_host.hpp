// What the host files of the C ABI (vtm_capi_*.cpp) share: the last-error helpers, the owners of device memory, streams
// and events, the plan, its small predicates, the request of a synthesis launch, and one helper per idiom that more than
// one of those files would otherwise write out.  Internal: never installed, nothing in it is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gama_vtm.h"
#include "vtm_design.hpp"
#include "vtm_kernels.hpp"
#include "vtm_tracks.hpp"

namespace gvtm::host {

// set the calling thread's last error (gvtm_last_error; defined next to it) and return the status
int fail(int status, const std::string& msg);
int fail_hip(hipError_t e, const char* what);

// Device memory with one owner, grown on demand; freed when the owner goes
struct DeviceBuffer {
	void* ptr = nullptr;
	size_t bytes = 0;
	DeviceBuffer() = default;
	DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
	DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
	{
		std::swap(ptr, o.ptr);
		std::swap(bytes, o.bytes);
		return *this;
	}
	~DeviceBuffer()
	{
		if (ptr) (void) hipFree(ptr);
	}
	template <typename T> T* as() const { return static_cast<T*>(ptr); }
	hipError_t ensure(size_t need)
	{
		if (need <= bytes) return hipSuccess;
		*this = DeviceBuffer(); // (the old memory goes before the new is taken)
		hipError_t e = hipMalloc(&ptr, need);
		if (e == hipSuccess) bytes = need;
		return e;
	}
};

// A HIP stream or event with one owner, destroyed when the owner goes
template <typename H, hipError_t (*Destroy)(H)>
struct Owned {
	H h = nullptr;
	Owned() = default;
	Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
	Owned& operator=(Owned&& o) noexcept
	{
		std::swap(h, o.h);
		return *this;
	}
	~Owned()
	{
		if (h) (void) Destroy(h);
	}
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// the two events around a timed launch: in the plan's pool, pending until gvtm_plan_take_kernel_ms, or destroyed
struct EventPair {
	Event start, stop;
};

// Makes the plan's device current for the duration of an entry point and gives the caller's device back afterwards.
class DeviceScope {
public:
	explicit DeviceScope(int device)
	{
		if (hipGetDevice(&previous_) != hipSuccess) previous_ = -1;
		status_ = (previous_ == device) ? hipSuccess : hipSetDevice(device);
		changed_ = status_ == hipSuccess && previous_ != device;
	}
	~DeviceScope()
	{
		if (changed_ && previous_ >= 0) (void) hipSetDevice(previous_);
	}
	DeviceScope(const DeviceScope&) = delete;
	DeviceScope& operator=(const DeviceScope&) = delete;
	// GVTM_OK, or the status of the failed switch with its message set
	int entered() const { return status_ == hipSuccess ? GVTM_OK : fail_hip(status_, "hipSetDevice"); }
private:
	int previous_ = -1;
	bool changed_ = false;
	hipError_t status_ = hipSuccess;
};

} // namespace gvtm::host

struct gvtm_plan {
	using DeviceBuffer = gvtm::host::DeviceBuffer;
	// one design per voice, voice 0 first (gvtm_plan_create_voices: several); d_consts, d_consts5 and d_wavetable hold one
	// block per voice, the FIR and the converter's tables (the same for every voice) one
	std::vector<gvtm::Design> designs;
	int device = 0;
	int precision = GVTM_PRECISION_F64;
	int rows = 0;       // utterances per workgroup; 0 = by batch size (a diagnostics build can force it)
	bool float5_voices = false; // made by gvtm_plan_create_model5_float_voices: a float model 5 plan that takes the voices entries
	// a float plan of the models 0 to 4 whose designed decimator is gvtm::kGlottalFirF32 bit for bit (create_plan compares):
	// its launches take the coefficients as literals (SynthArgs::fir_literals); a diagnostics build can clear it
	bool fir_literals = false;
	// a one-voice float plan that up-samples with at most gvtm::kSrcPhaseCap output phases: their number (create_plan), and on
	// a device plan the converter's coefficients by phase (upload_tables; 0 again where that allocation failed).  0: the
	// launches form the coefficients in the kernel.  A diagnostics build can clear it
	unsigned src_phases = 0;
	DeviceBuffer d_src_phase;
	// a one-voice plan whose wavetable never follows the amplitude (gvtm::static_wavetable; SynthArgs::static_wavetable); a
	// diagnostics build can clear it
	bool static_wavetable = false;
	// design tables on the device: double, or float (as designed) for GVTM_PRECISION_F32
	DeviceBuffer d_wavetable, d_fir, d_src_h, d_src_dh;
	DeviceBuffer d_consts, d_consts5; // gvtm::DeviceConstants, gvtm::Model5Constants (model 5 plans only)
	// the length of the targets' moving average and its reciprocal by voice (vtm_targets.hpp: targets_filter_length of the
	// voice's internal rate), what the kernels of gvtm_synthesize_targets_voices_device and, on model 5 plans,
	// gvtm_synthesize_targets_model5_voices_device read
	DeviceBuffer d_targets_N, d_targets_invN;
	// the noise source's samples by internal step (the same for every utterance), grown on demand; superseded buffers stay
	// allocated until the plan goes (a launch in flight on the caller's stream may still read them; the growth is
	// geometric, so together they are smaller than the live one)
	DeviceBuffer d_noise;
	size_t noise_len = 0;
	std::vector<DeviceBuffer> noise_retired;
	// scratch, one set per user, so that no call overwrites what another call's queued kernels still read:
	// the host entries' (one slice pipeline under two layouts, run_slices; each call drains its streams before it returns, so
	// the layouts never use the set at once): per utterance of the whole batch the frame counts, voice ids, out_counts, maxabs,
	// scales and the grouping's scratch; padded, the whole batch's staging; packed, two offset tables and three staging sets,
	// each one allocation that a slice carves into its packed frames, padded frames, padded samples and packed output
	// (gama_vtm.h: set_bytes), so that what is held is bounded by the slices and not by the batch; events-packed, the packed
	// layout's with the slice's events in the place of its packed frames, and the batch's two chunk tables and drift states ...
	struct {
		DeviceBuffer frames, voice_ids, counts, maxabs, scales, groups;
		DeviceBuffer params, audio, pcm;               // padded
		DeviceBuffer set[3], frame_offsets, sample_offsets; // packed, events-packed
		DeviceBuffer chunk_offsets, utt_chunks, drift;      // events-packed
		size_t limit = 0;                       // gvtm_plan_set_staging_limit; 0: none
		size_t slices = 0, largest_slice = 0;   // of the last packed call that ran
		size_t staging_bytes() const { return set[0].bytes + set[1].bytes + set[2].bytes; }
		void release_sets() { for (DeviceBuffer& s : set) s = DeviceBuffer(); }
		unsigned char* set_of(size_t i) const { return set[i % 3].as<unsigned char>(); } // slice i's: the sets rotate
	} host;
	// ... and the enqueue-only entries' (gvtm_synthesize_events_device's and gvtm_synthesize_modified_device's frames and frame counts, gvtm_synthesize_targets_device's
	// and gvtm_synthesize_targets_voices_device's step counts, the grouping of gvtm_synthesize_voices_device and of that entry, the merged event lists and their offsets of gvtm_synthesize_intonation_device): calls to
	// those on one plan must be ordered on one stream
	struct {
		DeviceBuffer params, frames, groups;
		DeviceBuffer events, event_offsets;
		// gvtm_synthesize_prosody_device's: what lies between its kernels (the merged lists go into the two above)
		struct {
			DeviceBuffer postures, rhythm_status, events, event_offsets, rule_data, rule_counts, onsets, points, point_offsets, status, list_ids;
		} prosody;
	} async;
	// gvtm_plan_set_voice_tracks: one designed track configuration per voice, and (device plans) the table the voice
	// variant of the tracks kernel reads; empty until the first call that succeeds
	std::vector<gvtm::TrackConstants> voice_tracks;
	DeviceBuffer d_voice_tracks;
	int compute_units = 0; // of the plan's device (the host entries cut big batches into slices that fill them once)
	// kernel timing (HIP events on the launch stream)
	bool timing = false;
	double* debug_taps = nullptr; // device pointer (diagnostics builds: gvtm_debug_set_taps)
	unsigned long long* phase_cycles = nullptr; // device pointer (diagnostics builds: gvtm_debug_set_phase_cycles)
	std::vector<gvtm::host::EventPair> pending, pool;
	// host-buffer entries: frames in on one stream, kernels on a second, samples out on a third (created on first use)
	gvtm::host::Stream h2d_stream, compute_stream, copy_stream;
	std::vector<gvtm::host::Event> slice_events; // three per slice: input arrived, output ready, output copied (recorded where sets rotate)

	int n_voices() const { return static_cast<int>(designs.size()); }
	// the shape of a launch of `batch` utterances (vtm_kernels.hpp: synth_launch_shape; forced_rows 0: the plan's own)
	// (targets: a launch from parameter targets, which model 5 has shapes of its own for)
	gvtm::LaunchShape launch_shape(size_t batch, int forced_rows, bool voices, int stream_ring = 0, bool fit = true, bool targets = false) const
	{
		return gvtm::synth_launch_shape(designs.data(), n_voices(), precision, batch, forced_rows ? forced_rows : rows, voices, stream_ring, fit, targets);
	}
	// the ring a stream keeps for voice v (not model 5): the one-row shape's, whatever shape a launch of the stream takes
	int stream_ring(int v) const { return gvtm::synth_launch_shape(&designs[v], 1, precision, 1, 1, false).ring; }
	// the ring the LDS of a stream's launches is sized for: the longest of the voices' (each voice keeps its own in the kernel)
	int longest_stream_ring() const
	{
		int xr = 0;
		for (int v = 0; v < n_voices(); ++v) xr = std::max(xr, stream_ring(v));
		return xr;
	}
	// the shape of a launch on behalf of a stream whose LDS holds rings of xr samples; a stream of a plan of several
	// voices launches the voice variant (gvtm_stream_create_voices); targets: a targets-fed run's launch (model 5: the targets
	// variant's shapes)
	gvtm::LaunchShape stream_launch_shape(size_t batch, int forced_rows, int xr, bool targets = false) const
	{
		return launch_shape(batch, forced_rows, n_voices() > 1, xr, true, targets);
	}
};

namespace gvtm::host {

// Host memory to a buffer of at least max(count, min_count) elements; no copy is issued for none.  min_count: for a buffer
// whose pointer goes to a kernel even when nothing is copied.  Synchronous; only ever called before an entry queues anything.
template <typename T>
int upload(DeviceBuffer& dst, const T* src, size_t count, const char* what, size_t min_count = 0)
{
	hipError_t e = dst.ensure(sizeof(T) * std::max(count, min_count));
	if (e == hipSuccess && count) e = hipMemcpy(dst.ptr, src, sizeof(T) * count, hipMemcpyHostToDevice);
	return e == hipSuccess ? GVTM_OK : fail_hip(e, what);
}

template <typename T>
int upload(DeviceBuffer& dst, const std::vector<T>& src, const char* what)
{
	return upload(dst, src.data(), src.size(), what);
}

// ... and back: count elements of a buffer to host memory
template <typename T>
int download(T* dst, const DeviceBuffer& src, size_t count, const char* what)
{
	const hipError_t e = count ? hipMemcpy(dst, src.ptr, sizeof(T) * count, hipMemcpyDeviceToHost) : hipSuccess;
	return e == hipSuccess ? GVTM_OK : fail_hip(e, what);
}

// Is there a HIP device at this index?  (what: the caller, which has no CPU path)
int check_device_index(int device, const char* what);

// The single-voice entry points on a plan of several voices: which voice would they synthesize?
inline int refuse_voices(const gvtm_plan* plan, const char* entry)
{
	return fail(GVTM_ERR_INVALID_ARGUMENT, std::string(entry) + ": the plan has " + std::to_string(plan->n_voices()) +
			" voices; use gvtm_synthesize_voices_* resp. gvtm_synthesize_events_voices_device (one voice id per utterance)");
}

// Everything that launches a kernel, on a design-only plan
inline int refuse_design_only()
{
	return fail(GVTM_ERR_NO_DEVICE, "design-only plan (GVTM_DEVICE_NONE): there is no CPU synthesis path");
}

// the most steps per frame among the plan's voices: what a launch is judged by, and what the noise table is as long as
inline unsigned max_control_steps(const gvtm_plan* plan)
{
	unsigned max_steps = 0;
	for (int v = 0; v < plan->n_voices(); ++v) max_steps = std::max(max_steps, plan->designs[v].k.control_steps);
	return max_steps;
}

// do utterances of `frames` frames fit the kernels' 31-bit step counter?
inline bool fits_step_counter(const gvtm_plan* plan, unsigned long long frames)
{
	return frames < (1ull << 31) && frames * max_control_steps(plan) + 4096ull < (1ull << 31);
}

// does the track configuration's control period agree with the plan's control rate?
inline bool control_period_matches(const gvtm_plan* plan, const gvtm::TrackConstants& tk)
{
	return static_cast<double>(tk.control_period) * plan->designs[0].control_rate == 1000.0;
}

// Track arguments for a batch of a plan of voices: from the plan its table on the device and the control period, which is
// every voice's (gvtm_plan_set_voice_tracks); the kernel variant's offset tables (and row_start) are the caller's to add
inline gvtm::TrackAppendArgs plan_track_args(const gvtm_plan* plan, const gvtm_event* d_events, const int32_t* d_voice_ids, size_t batch, size_t max_frames,
		float* d_params, int32_t* d_frame_counts, gvtm_drift_state* d_drift)
{
	gvtm::TrackAppendArgs args{};
	args.k.control_period = plan->voice_tracks[0].control_period;
	args.events = d_events;
	args.batch = batch;
	args.max_frames = max_frames;
	args.params = d_params;
	args.frame_counts = d_frame_counts;
	args.drift = d_drift;
	args.voice_k = static_cast<const gvtm::TrackConstants*>(plan->d_voice_tracks.ptr);
	args.voice_ids = d_voice_ids;
	args.n_voices = plan->n_voices();
	return args;
}

// What lies between the two launches of an events entry or of gvtm_synthesize_modified_device: the plan's frame buffer (the
// enqueue-only entries' scratch) and the frame counts, the caller's or the plan's
inline int events_scratch(gvtm_plan* plan, size_t batch, size_t max_frames, int32_t* d_frame_counts, float*& d_params, int32_t*& d_counts)
{
	hipError_t e;
	if ((e = plan->async.params.ensure(sizeof(float) * batch * std::max<size_t>(max_frames, 1) * GVTM_N_PARAM)) != hipSuccess) return fail_hip(e, "hipMalloc frames");
	if ((e = plan->async.frames.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frame counts");
	d_params = static_cast<float*>(plan->async.params.ptr);
	d_counts = d_frame_counts ? d_frame_counts : static_cast<int32_t*>(plan->async.frames.ptr);
	return GVTM_OK;
}

// the internal rate as the voice's model holds it (gvtm_info::internal_rate_hz): what the two moving averages' lengths follow
inline double internal_rate_hz(const gvtm::Design& dg)
{
	return dg.model5 ? dg.k5.sample_rate : static_cast<double>(dg.k.sample_rate);
}

// the samples finishSynthesis() leaves after n_steps internal steps (flush overrun included), whatever the control rate ...
inline size_t steps_output_count(const gvtm::Design& dg, size_t n_steps)
{
	const gvtm::DeviceConstants& k = dg.k;
	return static_cast<size_t>(gvtm::src_output_count(k.time_inc, k.pad, k.upsampling, static_cast<uint64_t>(n_steps)));
}

// ... and the row length that holds every utterance of up to max_steps steps
inline size_t steps_output_capacity(const gvtm::Design& dg, size_t max_steps)
{
	const gvtm::DeviceConstants& k = dg.k;
	return static_cast<size_t>(gvtm::src_output_capacity(k.time_inc, k.pad, k.upsampling, static_cast<uint64_t>(max_steps)));
}

inline size_t design_output_count(const gvtm::Design& dg, size_t n_frames)
{
	return steps_output_count(dg, n_frames * dg.k.control_steps);
}

inline size_t design_output_capacity(const gvtm::Design& dg, size_t max_frames)
{
	return steps_output_capacity(dg, max_frames * dg.k.control_steps);
}

// Host voice ids (the streams of several voices, the packed layouts): all of them in [0, n_voices), or the call is refused
inline int check_voice_ids(const gvtm_plan* plan, const int32_t* voice_ids, size_t batch)
{
	for (size_t b = 0; b < batch; ++b) {
		if (voice_ids[b] < 0 || voice_ids[b] >= plan->n_voices()) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, "utterance " + std::to_string(b) + ": voice id " + std::to_string(voice_ids[b]) + " outside [0, " +
					std::to_string(plan->n_voices()) + ")");
		}
	}
	return GVTM_OK;
}

// A batch's voice ids on the device, one per utterance: the caller's, or (null: the one voice of the plan) zeros
inline int upload_voice_ids(DeviceBuffer& dst, const int32_t* voice_ids, size_t batch)
{
	if (voice_ids) return upload(dst, voice_ids, batch, "upload voice ids");
	hipError_t e = dst.ensure(sizeof(int32_t) * batch);
	if (e == hipSuccess) e = hipMemset(dst.ptr, 0, sizeof(int32_t) * batch);
	return e == hipSuccess ? GVTM_OK : fail_hip(e, "zero voice ids");
}

// What a host offset table's first entry must be, and with it the sentences its refusals set
enum class FirstOffset {
	kZero,          // "<name> must start at 0 and not decrease", whichever half is broken; read even where n = 0
	kNotNegative,   // "<name> must not be negative", then "<name> must not decrease"
	kNotBelowZero,  // a negative first entry counts as a decrease: "<name> must not decrease"
};

// A host offset table of n + 1 entries, the bounds of n lists back to back: does it start as `first` asks, and never
// decrease?  (Without lists, n = 0, the two non-negative rules read nothing: such a table may be null.)
inline int check_offsets(const int64_t* table, size_t n, const char* name, FirstOffset first)
{
	const std::string decreases = std::string(name) + (first == FirstOffset::kZero ? " must start at 0 and not decrease" : " must not decrease");
	if (first == FirstOffset::kZero ? table[0] != 0 : n > 0 && table[0] < 0) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, first == FirstOffset::kNotNegative ? std::string(name) + " must not be negative" : decreases);
	}
	for (size_t i = 0; i < n; ++i) {
		if (table[i + 1] < table[i]) return fail(GVTM_ERR_INVALID_ARGUMENT, decreases);
	}
	return GVTM_OK;
}

// the frames the host's walk counts for the chunks [c0, c1) of a chunk table: what the tracks kernel generates for them
inline size_t chunks_frame_count(int control_period, const gvtm_event* events, const int64_t* chunk_offsets, int64_t c0, int64_t c1)
{
	size_t frames = 0;
	for (int64_t c = c0; c < c1; ++c) {
		frames += gvtm::tracks_frame_count(control_period, events + chunk_offsets[c], static_cast<size_t>(chunk_offsets[c + 1] - chunk_offsets[c]));
	}
	return frames;
}

// The frame counts the tracks kernel left on the device against those the host's walk predicted (expected(b): utterance
// b's), on which every size of the call was built
template <typename Expected>
int check_device_frame_counts(const DeviceBuffer& d_counts, size_t batch, Expected expected)
{
	std::vector<int32_t> counted(batch, 0);
	if (const int rc = download(counted.data(), d_counts, batch, "D2H frame counts"); rc != GVTM_OK) return rc;
	for (size_t b = 0; b < batch; ++b) {
		if (static_cast<int64_t>(counted[b]) != static_cast<int64_t>(expected(b))) return fail(GVTM_ERR_HIP, "internal error: the device's frame count differs from the host's");
	}
	return GVTM_OK;
}

// what a launch on behalf of a stream adds to the one-shot launch
struct StreamLaunch {
	unsigned char* d_state;
	size_t stride;
	int mode;     // gvtm::StreamMode
	int xr;       // the stream's ring length (one for all shapes; several voices: the longest of the plan's voices)
};

// what a launch from parameter targets (gvtm_synthesize_targets_device; a targets-fed stream's) has in the place of frames:
// the request's frame_counts are then its step counts, as the check kernel (the stream: the host) left them, and its
// max_frames the most steps of an utterance; a stream's points are its log, in absolute steps
struct TargetsLaunch {
	const int64_t* list_offsets;
	const int32_t* list_ids;   // or null
	const int32_t* point_steps;
	const float* point_values;
	int64_t N;                 // the filter's length and its reciprocal
	double invN;
	// a launch of several voices (LaunchRequest::voices): the two by voice, the plan's tables on the device; N and invN unused
	const int64_t* voice_N = nullptr;
	const double* voice_invN = nullptr;
};

// One synthesis launch: the device buffers of a gvtm_synthesize_*_device call, of a slice of the host entries or of a stream
struct LaunchRequest {
	const float* params;
	const int32_t* frame_counts;
	size_t batch, max_frames;
	float* audio;
	size_t audio_stride;
	int64_t* out_counts;
	float* maxabs;
	void* hip_stream;
	int rows = 0;                       // utterances per workgroup; 0 = by this launch's batch (gvtm_plan::launch_shape)
	bool voices = false;                // gvtm_synthesize_voices_*: voice_ids[b] is utterance b's voice
	const int32_t* voice_ids = nullptr;
	DeviceBuffer* groups = nullptr;     // voices: the caller's scratch for the row map, group voices and sort counts
	const StreamLaunch* sl = nullptr;   // or null: a one-shot launch
	const TargetsLaunch* targets = nullptr; // or null: a launch from frames
};

// Every synthesis launch, enqueue-only (vtm_capi_launch.cpp)
int launch_synthesis(gvtm_plan* plan, const LaunchRequest& r);
// a one-shot launch's rows hold max_frames frames of every voice
int check_audio_stride(const gvtm_plan* plan, size_t audio_stride, size_t max_frames, bool voices);
// The 16 sums of the targets filters as every utterance's block of a model 5 stream's device state holds them, out [batch][16]
// (vtm_capi_stream.cpp, which alone knows the structure; the diagnostics library's gvtm_debug_stream_targets_sums)
int stream_download_targets_sums(const gvtm_stream* stream, double* out);

// The device a rules object lives on, GVTM_DEVICE_NONE for a host-only one (vtm_capi_rules.cpp, which alone knows the structure)
int rules_device(const gvtm_rules* rules);

// What a listening stream needs of an analysis object (vtm_capi_analysis.cpp, which alone knows the structure): its facts,
// and the slices of gvtm_analyze_spectrum_device behind that entry's checks, enqueue-only on `stream` with the object's device
// current.  d_out_slots (or null) and out_stride: gvtm::AnalysisArgs::out_slots.
struct AnalysisFacts {
	int device;
	uint32_t sample_rate;
	size_t n_bins, W;
};
AnalysisFacts analysis_facts(const gvtm_analysis* analysis);
int analysis_enqueue(gvtm_analysis* analysis, const float* d_audio, size_t audio_stride, const int64_t* d_counts, const int64_t* d_first, size_t batch,
		size_t max_buffers, float* d_spectra, float* d_signal, int32_t* d_buffers_out, const int32_t* d_out_slots, size_t out_stride, hipStream_t stream);

} // namespace gvtm::host
