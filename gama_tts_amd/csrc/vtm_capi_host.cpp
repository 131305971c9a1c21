// C ABI of libgama_vtm.so, the host entries: host memory in, host memory out, through one slice pipeline (run_slices)
// under three layouts -- padded frames, packed frames, packed event lists.
#include <new>

#include "vtm_host.hpp"
#include "vtm_pack.hpp"

using namespace gvtm::host;

namespace {

// The host-buffer entries: frames in host memory -> samples in host memory, float32 (unscaled outputBuffer() samples) or
// int16 (scaled by 0.95 / max|x| and rounded as WAVEFileWriter::writeSample does, Controller.cpp:315-340,
// WAVEFileWriter.cpp:122-125 -- half the bytes over PCIe, which is what bounds this entry).
struct HostJob {
	const float* params;
	const int32_t* frame_counts;
	const int32_t* voice_ids; // null: the plan's one voice (gvtm_synthesize_batch_host*), else gvtm_synthesize_voices_host*
	size_t batch, max_frames;
	float* audio;      // float32 output [batch][stride], or null
	int16_t* pcm;      // int16 output [batch][stride], or null
	size_t stride;
	int64_t* out_counts;
	float* maxabs;
	float* scales;     // pcm only: the scale applied to each utterance, or null
};

// The shape of a whole batch of the host entries (every slice is launched in it), and in `machine` how many utterances fill
// the machine once in it (the rows the batch size picks: a launch still gives way to fewer where the LDS does not hold them)
gvtm::LaunchShape whole_batch_shape(const gvtm_plan* plan, size_t batch, size_t& machine)
{
	const gvtm::LaunchShape shape = plan->launch_shape(batch, 0, false, 0, false);
	machine = std::max<size_t>(1, static_cast<size_t>(shape.per_cu) * static_cast<size_t>(plan->compute_units > 0 ? plan->compute_units : 256));
	return shape;
}

// the grouping's scratch for a slice of `largest` utterances in any shape (rows <= 8), taken before the first slice: no
// launch regrows it under a queued kernel
hipError_t reserve_host_groups(gvtm_plan* plan, size_t largest)
{
	const size_t nv = static_cast<size_t>(plan->n_voices());
	return plan->host.groups.ensure(sizeof(int32_t) * ((largest + 8 + 8 * nv) + (largest + nv) + nv * gvtm::kGroupVoicesThreads));
}

// The slice pipeline of the host entries, three streams deep:
//     input(i + 1) on the H2D stream  ||  work(i) on the compute stream  ||  output(i - 1) on the copy stream
// A layout gives the three as callables that queue slice i's part on the stream they are handed (input and output: one
// copy, a hipError_t -- the events-packed layout's input also launches the tracks kernel behind its copy, its output may be
// two copies; work: kernels, a GVTM_* status with its message set), and two numbers.
// trail: slice i's output is queued behind the work of slice i + trail, or of the last slice.  With pageable host memory a
// device-to-host copy blocks the calling thread until its slice is done, so no output is queued before the kernels that may
// run beside it: trail = n_slices where the whole batch is staged on the device; 1, the least, where sets rotate, which
// needs the outputs queued in step (hipStreamWaitEvent on an event not recorded yet waits for nothing).  sets: slice i's
// input waits until the output of slice i - sets has left; 0: no output's leaving is recorded or waited for.  With
// page-locked host buffers (gvtm_host_alloc) all three really overlap; with pageable ones the runtime stages the copies
// itself and the call returns the same bytes.  The streams are drained when this returns, failed or not.
template <typename Input, typename Work, typename Output>
int run_slices(gvtm_plan* plan, size_t n_slices, size_t trail, size_t sets, const char* input_what, Input input, Work work, Output output)
{
	hipError_t e;
	for (Stream* st : {&plan->h2d_stream, &plan->compute_stream, &plan->copy_stream}) {
		if (!st->h && (e = hipStreamCreateWithFlags(&st->h, hipStreamNonBlocking)) != hipSuccess) return fail_hip(e, "hipStreamCreate");
	}
	const hipStream_t h2d_stream = plan->h2d_stream.h, compute_stream = plan->compute_stream.h, copy_stream = plan->copy_stream.h;
	while (plan->slice_events.size() < 3 * n_slices) {
		Event ev;
		if ((e = hipEventCreateWithFlags(&ev.h, hipEventDisableTiming)) != hipSuccess) return fail_hip(e, "hipEventCreate");
		plan->slice_events.push_back(std::move(ev));
	}
	enum { kArrived, kReady, kCopied };
	auto event = [&](size_t i, int which) { return plan->slice_events[3 * i + which].h; };
	auto queue_output = [&](size_t i) -> int {
		if ((e = hipStreamWaitEvent(copy_stream, event(i, kReady), 0)) != hipSuccess) return fail_hip(e, "hipStreamWaitEvent");
		if ((e = output(i, copy_stream)) != hipSuccess) return fail_hip(e, "D2H samples");
		if (sets && (e = hipEventRecord(event(i, kCopied), copy_stream)) != hipSuccess) return fail_hip(e, "hipEventRecord");
		return GVTM_OK;
	};
	auto queue_slice = [&](size_t i) -> int {
		if (sets && i >= sets && (e = hipStreamWaitEvent(h2d_stream, event(i - sets, kCopied), 0)) != hipSuccess) return fail_hip(e, "hipStreamWaitEvent");
		if ((e = input(i, h2d_stream)) != hipSuccess) return fail_hip(e, input_what);
		if ((e = hipEventRecord(event(i, kArrived), h2d_stream)) != hipSuccess) return fail_hip(e, "hipEventRecord");
		if ((e = hipStreamWaitEvent(compute_stream, event(i, kArrived), 0)) != hipSuccess) return fail_hip(e, "hipStreamWaitEvent");
		if (const int rc = work(i, compute_stream); rc != GVTM_OK) return rc;
		if ((e = hipEventRecord(event(i, kReady), compute_stream)) != hipSuccess) return fail_hip(e, "hipEventRecord");
		return i >= trail ? queue_output(i - trail) : GVTM_OK;
	};
	int rc = GVTM_OK;
	for (size_t i = 0; i < n_slices && rc == GVTM_OK; ++i) rc = queue_slice(i);
	for (size_t i = n_slices - std::min(trail, n_slices); i < n_slices && rc == GVTM_OK; ++i) rc = queue_output(i);
	if (rc == GVTM_OK && (e = hipStreamSynchronize(copy_stream)) != hipSuccess) rc = fail_hip(e, "vtm_synth_kernel execution / D2H samples");
	if (rc != GVTM_OK) {
		for (hipStream_t st : {h2d_stream, compute_stream, copy_stream}) (void) hipStreamSynchronize(st);
		return rc;
	}
	if ((e = hipStreamSynchronize(compute_stream)) != hipSuccess) return fail_hip(e, "vtm_synth_kernel execution");
	if ((e = hipStreamSynchronize(h2d_stream)) != hipSuccess) return fail_hip(e, input_what);
	return GVTM_OK;
}

// out_counts, maxabs and scales of the whole batch, from the host entries' scratch to the caller's arrays where given
int copy_back_results(gvtm_plan* plan, size_t batch, int64_t* out_counts, float* maxabs, float* scales)
{
	int rc = GVTM_OK;
	if (out_counts && (rc = download(out_counts, plan->host.counts, batch, "D2H counts")) != GVTM_OK) return rc;
	if (maxabs && (rc = download(maxabs, plan->host.maxabs, batch, "D2H maxabs")) != GVTM_OK) return rc;
	return scales ? download(scales, plan->host.scales, batch, "D2H scales") : GVTM_OK;
}

// The padded layout: params [batch][max_frames] in, rows [batch][stride] out, staged on the device for the whole batch.  A
// batch of at least two machine-fulls goes in slices of one machine-full each (rows x compute units utterances: every
// compute unit busy, in the shape the whole batch would use), each a region of the whole-batch buffers:
//     H2D frames(i + 1)  ||  kernel(i) [+ scale -> int16(i)]  ||  D2H samples, behind the last slice's kernels
int host_pipeline(gvtm_plan* plan, const HostJob& j)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	const bool voices = j.voice_ids != nullptr;
	if (!voices && plan->n_voices() > 1) return refuse_voices(plan, j.pcm ? "gvtm_synthesize_batch_host_pcm16" : "gvtm_synthesize_batch_host");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	const size_t batch = j.batch, max_frames = j.max_frames, audio_stride = j.stride;
	if (batch == 0) return GVTM_OK;
	if (!j.audio && !j.pcm) return fail(GVTM_ERR_INVALID_ARGUMENT, "null output buffer");
	if (max_frames > 0 && !j.params) return fail(GVTM_ERR_INVALID_ARGUMENT, "null params with max_frames > 0");
	// (with voices too the single-voice sentence)
	int rc = check_audio_stride(plan, audio_stride, max_frames, false);
	if (rc != GVTM_OK) return rc;
	// A frame count outside [0, max_frames] fails THAT utterance (out_counts[b] = -1, no samples); the others are
	// synthesized.  The device sees it as an empty utterance.
	std::vector<int32_t> sane;
	std::vector<size_t> bad;
	try {
		if (j.frame_counts) {
			for (size_t b = 0; b < batch; ++b) {
				if (j.frame_counts[b] < 0 || static_cast<size_t>(j.frame_counts[b]) > max_frames) {
					if (sane.empty()) sane.assign(j.frame_counts, j.frame_counts + batch);
					sane[b] = 0;
					bad.push_back(b);
				}
			}
		}
		// a voice id outside [0, n_voices) fails that utterance the same way (the device leaves it out of the row map)
		if (voices) {
			for (size_t b = 0; b < batch; ++b) {
				if (j.voice_ids[b] < 0 || j.voice_ids[b] >= plan->n_voices()) bad.push_back(b);
			}
		}
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
	const int32_t* const counts_in = sane.empty() ? j.frame_counts : sane.data();
	size_t machine;
	const gvtm::LaunchShape shape_all = whole_batch_shape(plan, batch, machine);
	const size_t slice = batch >= 2 * machine ? machine : batch;
	const size_t n_slices = (batch + slice - 1) / slice;

	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	hipError_t e;
	const size_t row_in = max_frames * GVTM_N_PARAM;
	const size_t pbytes = sizeof(float) * batch * row_in;
	auto& sc = plan->host;
	if ((e = sc.params.ensure(pbytes ? pbytes : 16)) != hipSuccess) return fail_hip(e, "hipMalloc params");
	if ((e = sc.audio.ensure(std::max<size_t>(16, sizeof(float) * batch * audio_stride))) != hipSuccess) return fail_hip(e, "hipMalloc audio");
	if ((e = sc.counts.ensure(sizeof(int64_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc counts");
	if ((e = sc.maxabs.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc maxabs");
	if (counts_in && (rc = upload(sc.frames, counts_in, batch, "upload frame counts")) != GVTM_OK) return rc;
	if (voices && (rc = upload(sc.voice_ids, j.voice_ids, batch, "upload voice ids")) != GVTM_OK) return rc;
	if (j.pcm && (e = sc.pcm.ensure(std::max<size_t>(16, sizeof(int16_t) * batch * audio_stride))) != hipSuccess) return fail_hip(e, "hipMalloc pcm");
	if (j.pcm && (e = sc.scales.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc scales");
	if (voices && (e = reserve_host_groups(plan, slice)) != hipSuccess) return fail_hip(e, "hipMalloc row map");

	float* const d_params = sc.params.as<float>();
	float* const d_audio = sc.audio.as<float>();
	int16_t* const d_pcm = sc.pcm.as<int16_t>();
	int64_t* const d_counts = sc.counts.as<int64_t>();
	float* const d_maxabs = sc.maxabs.as<float>();
	// rows come back zero beyond their sample count (the staging buffers are reused between calls; the voices of a mixed
	// batch give different counts)
	const bool ragged = counts_in != nullptr || voices || audio_stride > gvtm_output_count(plan, max_frames);

	// slice i: utterances [lo, lo + n)
	auto count_of = [&](size_t i) { return std::min(slice, batch - i * slice); };
	auto input = [&](size_t i, hipStream_t stream) {
		const size_t lo = i * slice;
		return pbytes ? hipMemcpyAsync(d_params + lo * row_in, j.params + lo * row_in, sizeof(float) * count_of(i) * row_in, hipMemcpyHostToDevice, stream) : hipSuccess;
	};
	auto work = [&](size_t i, hipStream_t stream) {
		const size_t lo = i * slice, n = count_of(i);
		const hipError_t we = !ragged ? hipSuccess : j.pcm ? hipMemsetAsync(d_pcm + lo * audio_stride, 0, sizeof(int16_t) * n * audio_stride, stream)
		                                                   : hipMemsetAsync(d_audio + lo * audio_stride, 0, sizeof(float) * n * audio_stride, stream);
		if (we != hipSuccess) return fail_hip(we, "hipMemsetAsync");
		int wrc = launch_synthesis(plan, LaunchRequest{d_params + lo * row_in, counts_in ? sc.frames.as<int32_t>() + lo : nullptr, n, max_frames, d_audio + lo * audio_stride,
				audio_stride, d_counts + lo, d_maxabs + lo, stream, shape_all.forced, voices, voices ? sc.voice_ids.as<int32_t>() + lo : nullptr, &sc.groups});
		// (normalize takes at most 65535 utterances per launch: a slice is far below that unless the batch is one slice)
		for (size_t q = 0; j.pcm && q < n && wrc == GVTM_OK; q += 32768) {
			const size_t m = std::min<size_t>(32768, n - q);
			wrc = gvtm_normalize_batch_device(plan, d_audio + (lo + q) * audio_stride, m, audio_stride, d_counts + lo + q, d_maxabs + lo + q, nullptr,
					d_pcm + (lo + q) * audio_stride, sc.scales.as<float>() + lo + q, stream);
		}
		return wrc;
	};
	auto output = [&](size_t i, hipStream_t stream) {
		const size_t lo = i * slice, n = count_of(i);
		if (j.pcm) return hipMemcpyAsync(j.pcm + lo * audio_stride, d_pcm + lo * audio_stride, sizeof(int16_t) * n * audio_stride, hipMemcpyDeviceToHost, stream);
		return hipMemcpyAsync(j.audio + lo * audio_stride, d_audio + lo * audio_stride, sizeof(float) * n * audio_stride, hipMemcpyDeviceToHost, stream);
	};
	if ((rc = run_slices(plan, n_slices, n_slices, 0, "H2D params", input, work, output)) != GVTM_OK) return rc;
	if ((rc = copy_back_results(plan, batch, j.out_counts, j.maxabs, j.scales)) != GVTM_OK) return rc;
	for (size_t b : bad) {
		if (j.out_counts) j.out_counts[b] = -1;
		if (j.maxabs) j.maxabs[b] = 0.0f;
		if (j.scales) j.scales[b] = 0.0f;
		if (j.audio) std::fill(j.audio + b * audio_stride, j.audio + (b + 1) * audio_stride, 0.0f);
		if (j.pcm) std::fill(j.pcm + b * audio_stride, j.pcm + (b + 1) * audio_stride, int16_t(0));
	}
	if (!bad.empty()) (void) fail(GVTM_OK, voices ? "frame_counts entry outside [0, max_frames] or voice id outside [0, n_voices): those utterances have out_counts = -1"
	                                                : "frame_counts entry outside [0, max_frames]: those utterances have out_counts = -1");
	return GVTM_OK;
}

/* ---------------------------------------------------------------------------------------------
 * Ragged batches, packed in and packed out (include/gama_vtm.h, "Ragged batches").
 */

size_t round_up_packed(size_t n)
{
	return (n + GVTM_PACKED_ALIGN - 1) / GVTM_PACKED_ALIGN * GVTM_PACKED_ALIGN;
}

// The tables of a packed batch, all host memory, checked in the order the header lists the refusals; on success
// offsets[b] is where utterance b starts in the packed output and offsets[batch] the capacity it needs.
int packed_layout(const gvtm_plan* plan, const int64_t* frame_offsets, const int32_t* voice_ids, size_t batch, std::vector<int64_t>& offsets)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	offsets.assign(batch + 1, 0);
	if (batch == 0) return GVTM_OK;
	if (!frame_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null frame_offsets");
	int rc = check_offsets(frame_offsets, batch, "frame_offsets", FirstOffset::kZero);
	if (rc == GVTM_OK && voice_ids) rc = check_voice_ids(plan, voice_ids, batch);
	if (rc != GVTM_OK) return rc;
	if (!voice_ids && plan->n_voices() > 1) return fail(GVTM_ERR_INVALID_ARGUMENT, "null voice ids: the plan has " + std::to_string(plan->n_voices()) + " voices (one voice id per utterance)");
	for (size_t b = 0; b < batch; ++b) {
		const unsigned long long frames = static_cast<unsigned long long>(frame_offsets[b + 1] - frame_offsets[b]);
		// (as launch_synthesis judges a launch: by the voice with the most steps per frame)
		if (!fits_step_counter(plan, frames)) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, "utterance " + std::to_string(b) + ": frames * control_steps does not fit the 31-bit step counter");
		}
		const size_t count = design_output_count(plan->designs[voice_ids ? voice_ids[b] : 0], static_cast<size_t>(frames));
		offsets[b + 1] = static_cast<int64_t>(round_up_packed(static_cast<size_t>(offsets[b]) + count));
	}
	return GVTM_OK;
}

// What a packed call returns, whichever layout its input has
struct PackedOutputs {
	float* audio;     // float32 output, or null
	int16_t* pcm;     // int16 output, or null
	bool to_pcm;      // which of the two is due
	size_t capacity;
	int64_t* sample_offsets_out;
	int64_t* out_counts;
	float* maxabs;
	float* scales;    // pcm only
	void* samples() const { return to_pcm ? static_cast<void*>(pcm) : static_cast<void*>(audio); }
	size_t width() const { return to_pcm ? sizeof(int16_t) : sizeof(float); } // bytes per sample out
};

struct PackedJob {
	const float* frames;
	const int64_t* frame_offsets;
	const int32_t* voice_ids; // null: the plan's one voice through the single-voice launch, else the voices launch
	size_t batch;
	PackedOutputs out;
};

// Between the tables of a packed batch (packed_layout, events_packed_layout) and its slices, the refusals in the header's
// order: a null output buffer; own_first; a capacity below the layout's (query: the entry that tells it); own_last (the
// layout's own refusals where they are due, empty where not); a design-only plan.  Then the empty batch, which is over
// here, and a batch too large.  Past these, shape_all is the shape every slice is launched in, as host_pipeline's, and
// machine the utterances that fill the machine once in it.
int packed_prologue(const gvtm_plan* plan, const PackedOutputs& o, size_t batch, const std::vector<int64_t>& offsets, const char* query,
		const std::string& own_first, const std::string& own_last, gvtm::LaunchShape& shape_all, size_t& machine)
{
	if (batch != 0) {
		if (!o.samples()) return fail(GVTM_ERR_INVALID_ARGUMENT, o.to_pcm ? "null pcm buffer" : "null audio buffer");
		if (!own_first.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, own_first);
		if (o.capacity < static_cast<size_t>(offsets[batch])) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(o.capacity) + " below " + query + " (" + std::to_string(offsets[batch]) + " samples)");
		}
		if (!own_last.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, own_last);
	}
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (batch == 0) {
		if (o.sample_offsets_out) o.sample_offsets_out[0] = 0;
		return GVTM_OK;
	}
	if (batch > 0x3fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large");
	shape_all = whole_batch_shape(plan, batch, machine);
	return GVTM_OK;
}

// utterances [lo, hi) in one staging set: its longest utterance, the rows' length and the bytes of the header's formula.
// The set, carved in this order: the slice's input (packed frames; events-packed: its events, rounded up to 64 bytes),
// padded frames, padded samples, packed output and (events-packed with frames_out) the packed frames that go back
struct PackedSlice {
	size_t lo, hi, max_frames, stride, in_bytes, rows_bytes, audio_bytes, out_bytes, frames_bytes;
	size_t bytes() const { return in_bytes + rows_bytes + audio_bytes + out_bytes + frames_bytes; }
	float* rows(unsigned char* set) const { return reinterpret_cast<float*>(set + in_bytes); }
	float* audio(unsigned char* set) const { return reinterpret_cast<float*>(set + in_bytes + rows_bytes); }
	unsigned char* out(unsigned char* set) const { return set + in_bytes + rows_bytes + audio_bytes; }
	float* frames(unsigned char* set) const { return reinterpret_cast<float*>(set + in_bytes + rows_bytes + audio_bytes + out_bytes); }
};

// the part of a set every packed layout has (in_bytes and frames_bytes are the layout's to add); width: bytes per sample out
PackedSlice packed_slice(const gvtm_plan* plan, size_t width, const std::vector<int64_t>& offsets, size_t lo, size_t hi, size_t max_frames)
{
	PackedSlice s{};
	s.lo = lo, s.hi = hi, s.max_frames = max_frames;
	// (the capacity, not the count of max_frames frames: a shorter utterance that hits the flush overrun is longer)
	s.stride = round_up_packed(gvtm_voices_output_capacity(plan, max_frames));
	const size_t n = hi - lo;
	s.rows_bytes = sizeof(float) * GVTM_N_PARAM * n * max_frames;
	s.audio_bytes = sizeof(float) * n * s.stride;
	s.out_bytes = width * static_cast<size_t>(offsets[hi] - offsets[lo]);
	return s;
}

// The slices of a packed batch, on the host, before any device work: utterances in the caller's order, a slice closed when
// the next utterance would exceed one machine-full or (with a limit) a third of the limit.  slice_of(lo, hi, max_frames):
// the layout's accounting of utterances [lo, hi).  longest: the most frames any utterance has.
template <typename SliceOf>
int cut_slices(const gvtm_plan* plan, const int64_t* frame_offsets, size_t batch, size_t machine, SliceOf slice_of, std::vector<PackedSlice>& slices, size_t& longest)
{
	const size_t limit = plan->host.limit, set_limit = limit / 3;
	longest = 0;
	for (size_t lo = 0; lo < batch;) {
		size_t max_frames = static_cast<size_t>(frame_offsets[lo + 1] - frame_offsets[lo]);
		PackedSlice s = slice_of(lo, lo + 1, max_frames);
		if (limit && s.bytes() > set_limit) {
			return fail(GVTM_ERR_OUT_OF_MEMORY, "utterance " + std::to_string(lo) + " needs a staging set of " + std::to_string(s.bytes()) +
					" bytes, three of them " + std::to_string(3 * s.bytes()) + "; the staging limit is " + std::to_string(limit));
		}
		for (size_t hi = lo + 2; hi <= batch && hi - lo <= machine; ++hi) {
			const size_t f = std::max(max_frames, static_cast<size_t>(frame_offsets[hi] - frame_offsets[hi - 1]));
			const PackedSlice wider = slice_of(lo, hi, f);
			if (limit && wider.bytes() > set_limit) break;
			s = wider, max_frames = f;
		}
		longest = std::max(longest, s.max_frames);
		slices.push_back(s);
		lo = s.hi;
	}
	return GVTM_OK;
}

// What every packed layout holds on the device before its first slice: the staging sets, the batch's small arrays (the two
// offset tables and the voice ids uploaded), the grouping's scratch and, for the longest utterance, the noise table.  With
// those in place the caller gets the sample offsets: from here on the call is device work
int stage_packed_batch(gvtm_plan* plan, const std::vector<PackedSlice>& slices, size_t longest, size_t batch, const int64_t* frame_offsets,
		const std::vector<int64_t>& offsets, const int32_t* voice_ids, const PackedOutputs& o)
{
	auto& sc = plan->host;
	const bool voices = voice_ids != nullptr;
	const size_t limit = sc.limit, set_limit = limit / 3;
	const size_t n_sets = std::min<size_t>(3, slices.size());
	size_t set_bytes = 16, largest = 0;
	for (const PackedSlice& s : slices) set_bytes = std::max(set_bytes, s.bytes()), largest = std::max(largest, s.hi - s.lo);
	hipError_t e;
	// (sets only grow; under a limit none may stay larger than its third)
	if (limit && std::max({sc.set[0].bytes, sc.set[1].bytes, sc.set[2].bytes}) > set_limit) plan->host.release_sets();
	for (size_t q = 0; q < n_sets; ++q) {
		if ((e = sc.set[q].ensure(set_bytes)) != hipSuccess) return e == hipErrorOutOfMemory ? fail(GVTM_ERR_OUT_OF_MEMORY, "hipMalloc staging set: out of memory") : fail_hip(e, "hipMalloc staging set");
	}
	int rc = upload(sc.frame_offsets, frame_offsets, batch + 1, "upload frame offsets");
	if (rc == GVTM_OK) rc = upload(sc.sample_offsets, offsets, "upload sample offsets");
	if (rc == GVTM_OK && voices) rc = upload(sc.voice_ids, voice_ids, batch, "upload voice ids");
	if (rc != GVTM_OK) return rc;
	if ((e = sc.frames.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frame counts");
	if ((e = sc.counts.ensure(sizeof(int64_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc counts");
	if ((e = sc.maxabs.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc maxabs");
	if (o.to_pcm && (e = sc.scales.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc scales");
	if (voices && (e = reserve_host_groups(plan, largest)) != hipSuccess) return fail_hip(e, "hipMalloc row map");
	// the noise table once, for the longest utterance: no slice regrows it in the middle of the pipeline
	if ((rc = gvtm_plan_reserve(plan, longest)) != GVTM_OK) return rc;
	sc.slices = slices.size(), sc.largest_slice = largest;
	if (o.sample_offsets_out) std::copy(offsets.begin(), offsets.end(), o.sample_offsets_out);
	return GVTM_OK;
}

// Behind a slice's padded frames and frame counts: the synthesis launch on its rows, then its samples packed into the set's
// output region (int16: scaled and rounded on the way)
int synthesize_and_pack(gvtm_plan* plan, const PackedSlice& s, unsigned char* set, bool pcm, bool voices, int forced_rows, hipStream_t stream)
{
	auto& sc = plan->host;
	const size_t n = s.hi - s.lo;
	int64_t* const d_counts = sc.counts.as<int64_t>() + s.lo;
	float* const d_maxabs = sc.maxabs.as<float>() + s.lo;
	const LaunchRequest request{s.rows(set), sc.frames.as<int32_t>() + s.lo, n, s.max_frames, s.audio(set), s.stride, d_counts, d_maxabs, stream, forced_rows, voices,
			voices ? sc.voice_ids.as<int32_t>() + s.lo : nullptr, &sc.groups};
	if (const int rc = launch_synthesis(plan, request); rc != GVTM_OK) return rc;
	const hipError_t e = gvtm::launch_pack_samples(gvtm::PackSamplesArgs{s.audio(set), d_counts, d_maxabs, sc.sample_offsets.as<int64_t>() + s.lo,
			pcm ? nullptr : reinterpret_cast<float*>(s.out(set)), pcm ? reinterpret_cast<int16_t*>(s.out(set)) : nullptr, pcm ? sc.scales.as<float>() + s.lo : nullptr, n, s.stride},
			stream);
	return e == hipSuccess ? GVTM_OK : fail_hip(e, "vtm_pack_samples_kernel launch");
}

// a slice's packed output leaves: one contiguous range [offset[lo], offset[hi]) of the caller's buffer (`host`: its start)
hipError_t copy_out_packed(const PackedSlice& s, unsigned char* set, void* host, size_t width, const std::vector<int64_t>& offsets, hipStream_t stream)
{
	if (!s.out_bytes) return hipSuccess;
	return hipMemcpyAsync(static_cast<unsigned char*>(host) + width * static_cast<size_t>(offsets[s.lo]), s.out(set), s.out_bytes, hipMemcpyDeviceToHost, stream);
}

// The packed layout: utterances in the caller's order, in contiguous slices of at most one machine-full and (with a limit)
// of at most a third of the limit, three staging sets deep:
//     H2D packed frames(i + 1)  ||  unpack + synthesis + pack(i)  ||  D2H packed output(i - 1)
// Slice i uses set i % 3; its frames go up once the output of slice i - 3 has left.
int packed_pipeline(gvtm_plan* plan, const PackedJob& j)
{
	std::vector<int64_t> offsets;
	try {
		int rc = packed_layout(plan, j.frame_offsets, j.voice_ids, j.batch, offsets);
		if (rc != GVTM_OK) return rc;
		const size_t batch = j.batch;
		const bool voices = j.voice_ids != nullptr, pcm = j.out.to_pcm;
		size_t machine, longest;
		gvtm::LaunchShape shape_all;
		const char* const no_frames = batch && j.frame_offsets[batch] > 0 && !j.frames ? "null frames" : "";
		if ((rc = packed_prologue(plan, j.out, batch, offsets, "gvtm_packed_sample_offsets", no_frames, "", shape_all, machine)) != GVTM_OK || batch == 0) return rc;
		auto& sc = plan->host;
		const size_t width = j.out.width();
		std::vector<PackedSlice> slices;
		auto slice_of = [&](size_t lo, size_t hi, size_t max_frames) {
			PackedSlice s = packed_slice(plan, width, offsets, lo, hi, max_frames);
			s.in_bytes = sizeof(float) * GVTM_N_PARAM * static_cast<size_t>(j.frame_offsets[hi] - j.frame_offsets[lo]);
			return s;
		};
		if ((rc = cut_slices(plan, j.frame_offsets, batch, machine, slice_of, slices, longest)) != GVTM_OK) return rc;

		DeviceScope scope(plan->device);
		if ((rc = scope.entered()) != GVTM_OK) return rc;
		if ((rc = stage_packed_batch(plan, slices, longest, batch, j.frame_offsets, offsets, j.voice_ids, j.out)) != GVTM_OK) return rc;

		auto input = [&](size_t i, hipStream_t stream) {
			const PackedSlice& s = slices[i];
			return s.in_bytes ? hipMemcpyAsync(sc.set_of(i), j.frames + GVTM_N_PARAM * static_cast<size_t>(j.frame_offsets[s.lo]), s.in_bytes, hipMemcpyHostToDevice, stream) : hipSuccess;
		};
		auto work = [&](size_t i, hipStream_t stream) -> int {
			const PackedSlice& s = slices[i];
			const hipError_t we = gvtm::launch_unpack_frames(gvtm::UnpackFramesArgs{reinterpret_cast<float*>(sc.set_of(i)), sc.frame_offsets.as<int64_t>() + s.lo, s.rows(sc.set_of(i)),
					sc.frames.as<int32_t>() + s.lo, s.hi - s.lo, s.max_frames}, stream);
			if (we != hipSuccess) return fail_hip(we, "vtm_unpack_frames_kernel launch");
			return synthesize_and_pack(plan, s, sc.set_of(i), pcm, voices, shape_all.forced, stream);
		};
		auto output = [&](size_t i, hipStream_t stream) {
			return copy_out_packed(slices[i], sc.set_of(i), j.out.samples(), width, offsets, stream);
		};
		if ((rc = run_slices(plan, slices.size(), 1, 3, "H2D frames", input, work, output)) != GVTM_OK) return rc;
		return copy_back_results(plan, batch, j.out.out_counts, j.out.maxabs, j.out.scales);
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

// Event lists in, packed samples out: the chunk tables of a batch, all host memory
struct EventsPackedJob {
	const gvtm_event* events;
	const int64_t* chunk_offsets; // [n_chunks + 1]
	const int64_t* utt_chunks;    // [batch + 1]
	const int32_t* voice_ids;     // null: the plan's one voice through the single-voice launch (the tracks kernel gets zeros)
	size_t batch;
	PackedOutputs out;
	int64_t* frame_offsets_out;
	float* frames_out;            // packed frames [frame_offsets[batch]][16], or null
	size_t frames_capacity;       // in frames
	gvtm_drift_state* drift;      // [batch] in/out, or null
};

// The tables of an events-packed batch, checked in the order the header lists the refusals, up to the 31-bit counter; on
// success frame_offsets is the prefix sum of the frames the host's walk counts per utterance (gvtm::tracks_frame_count over
// its chunks, as gvtm_stream_push_events) and offsets the packed layout of those (packed_layout)
int events_packed_layout(const gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks, const int32_t* voice_ids,
		size_t batch, std::vector<int64_t>& frame_offsets, std::vector<int64_t>& offsets)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, "gvtm_synthesize_events_packed_host: the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	frame_offsets.assign(batch + 1, 0);
	offsets.assign(batch + 1, 0);
	if (batch == 0) return GVTM_OK;
	if (!chunk_offsets || !utt_chunks) return fail(GVTM_ERR_INVALID_ARGUMENT, "null chunk_offsets or utt_chunks");
	// (read before the table is judged, but only to tell whether there are chunks: nothing is indexed with it yet)
	if (utt_chunks[batch] > 0 && !events) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events while chunks are present");
	int rc = check_offsets(utt_chunks, batch, "utt_chunks", FirstOffset::kZero);
	if (rc == GVTM_OK) rc = check_offsets(chunk_offsets, static_cast<size_t>(utt_chunks[batch]), "chunk_offsets", FirstOffset::kZero);
	if (rc != GVTM_OK) return rc;
	const int cp = plan->voice_tracks[0].control_period; // (every voice's is the plan's: gvtm_plan_set_voice_tracks)
	for (size_t b = 0; b < batch; ++b) {
		frame_offsets[b + 1] = frame_offsets[b] + static_cast<int64_t>(chunks_frame_count(cp, events, chunk_offsets, utt_chunks[b], utt_chunks[b + 1]));
	}
	// the ids and the 31-bit counter, as the packed entry checks them
	return packed_layout(plan, frame_offsets.data(), voice_ids, batch, offsets);
}

// The events-packed layout: the packed layout with a slice's events in the place of its packed frames and the tracks kernel
// in the place of the unpack pass:
//     H2D events + tracks(i + 1)  ||  synthesis + pack(i)  ||  D2H packed output [+ packed frames](i - 1)
// The events of a slice are one contiguous range of the caller's; the two chunk tables, the ids and the drift states are the
// batch's, uploaded once and indexed per slice.
int events_packed_pipeline(gvtm_plan* plan, const EventsPackedJob& j)
{
	std::vector<int64_t> frame_offsets, offsets;
	try {
		int rc = events_packed_layout(plan, j.events, j.chunk_offsets, j.utt_chunks, j.voice_ids, j.batch, frame_offsets, offsets);
		if (rc != GVTM_OK) return rc;
		const size_t batch = j.batch;
		const bool voices = j.voice_ids != nullptr, pcm = j.out.to_pcm;
		size_t machine, longest;
		gvtm::LaunchShape shape_all;
		const std::string frames_short = !j.frames_out || j.frames_capacity >= static_cast<size_t>(frame_offsets[batch]) ? ""
				: "frames_capacity " + std::to_string(j.frames_capacity) + " below the layout's " + std::to_string(frame_offsets[batch]) + " frames";
		rc = packed_prologue(plan, j.out, batch, offsets, "gvtm_events_packed_layout", "", frames_short, shape_all, machine);
		if (rc == GVTM_OK && batch == 0 && j.frame_offsets_out) j.frame_offsets_out[0] = 0;
		if (rc != GVTM_OK || batch == 0) return rc;
		auto& sc = plan->host;
		const size_t width = j.out.width();
		const size_t n_chunks = static_cast<size_t>(j.utt_chunks[batch]);
		// utterance b's first event, batch-wide (b = batch: the end of the last one's)
		auto event_of = [&](size_t b) { return static_cast<size_t>(j.chunk_offsets[j.utt_chunks[b]]); };
		std::vector<PackedSlice> slices;
		auto slice_of = [&](size_t lo, size_t hi, size_t max_frames) {
			PackedSlice s = packed_slice(plan, width, offsets, lo, hi, max_frames);
			// (the rows behind the events are stored 16 bytes at a time)
			s.in_bytes = (sizeof(gvtm_event) * (event_of(hi) - event_of(lo)) + 63) / 64 * 64;
			if (j.frames_out) s.frames_bytes = sizeof(float) * GVTM_N_PARAM * static_cast<size_t>(frame_offsets[hi] - frame_offsets[lo]);
			return s;
		};
		if ((rc = cut_slices(plan, frame_offsets.data(), batch, machine, slice_of, slices, longest)) != GVTM_OK) return rc;

		DeviceScope scope(plan->device);
		if ((rc = scope.entered()) != GVTM_OK) return rc;
		if ((rc = stage_packed_batch(plan, slices, longest, batch, frame_offsets.data(), offsets, j.voice_ids, j.out)) != GVTM_OK) return rc;
		if ((rc = upload(sc.chunk_offsets, j.chunk_offsets, n_chunks + 1, "upload chunk offsets")) != GVTM_OK) return rc;
		if ((rc = upload(sc.utt_chunks, j.utt_chunks, batch + 1, "upload utterance chunks")) != GVTM_OK) return rc;
		// (one voice: the tracks kernel still reads an id per utterance, the one voice's)
		if (!voices && (rc = upload_voice_ids(sc.voice_ids, nullptr, batch)) != GVTM_OK) return rc;
		if (j.drift && (rc = upload(sc.drift, j.drift, batch, "upload drift states")) != GVTM_OK) return rc;
		if (j.frame_offsets_out) std::copy(frame_offsets.begin(), frame_offsets.end(), j.frame_offsets_out);

		// slice i's events go up and its frames are generated behind them on the H2D stream: the walk is a chain of dependent
		// steps (as long as the slice's longest list, however few the utterances) that one wavefront per two utterances runs, so it
		// runs beside the synthesis kernels of the slice before instead of in front of its own
		auto input = [&](size_t i, hipStream_t stream) {
			const PackedSlice& s = slices[i];
			const size_t first = event_of(s.lo), n_events = event_of(s.hi) - first;
			const hipError_t ie = n_events ? hipMemcpyAsync(sc.set_of(i), j.events + first, sizeof(gvtm_event) * n_events, hipMemcpyHostToDevice, stream) : hipSuccess;
			if (ie != hipSuccess) return ie;
			gvtm::TrackSliceArgs ta{};
			static_cast<gvtm::TrackChunksArgs&>(ta) = plan_track_args(plan, reinterpret_cast<const gvtm_event*>(sc.set_of(i)), sc.voice_ids.as<int32_t>() + s.lo, s.hi - s.lo,
					s.max_frames, s.rows(sc.set_of(i)), sc.frames.as<int32_t>() + s.lo, j.drift ? sc.drift.as<gvtm_drift_state>() + s.lo : nullptr);
			ta.chunk_offsets = sc.chunk_offsets.as<int64_t>();
			ta.utt_chunks = sc.utt_chunks.as<int64_t>() + s.lo;
			ta.event_base = static_cast<int64_t>(first);
			ta.packed = j.frames_out ? s.frames(sc.set_of(i)) : nullptr;
			ta.frame_offsets = sc.frame_offsets.as<int64_t>() + s.lo;
			return gvtm::launch_tracks(ta, stream);
		};
		auto work = [&](size_t i, hipStream_t stream) -> int {
			return synthesize_and_pack(plan, slices[i], sc.set_of(i), pcm, voices, shape_all.forced, stream);
		};
		auto output = [&](size_t i, hipStream_t stream) {
			const PackedSlice& s = slices[i];
			const hipError_t oe = copy_out_packed(s, sc.set_of(i), j.out.samples(), width, offsets, stream);
			if (oe != hipSuccess || !s.frames_bytes) return oe;
			return hipMemcpyAsync(j.frames_out + GVTM_N_PARAM * static_cast<size_t>(frame_offsets[s.lo]), s.frames(sc.set_of(i)), s.frames_bytes, hipMemcpyDeviceToHost, stream);
		};
		if ((rc = run_slices(plan, slices.size(), 1, 3, "H2D events / track generation launch", input, work, output)) != GVTM_OK) return rc;
		if ((rc = copy_back_results(plan, batch, j.out.out_counts, j.out.maxabs, j.out.scales)) != GVTM_OK) return rc;
		if (j.drift && (rc = download(j.drift, sc.drift, batch, "D2H drift states")) != GVTM_OK) return rc;
		// what the tracks kernel counted against what the layout was built on
		return check_device_frame_counts(sc.frames, batch, [&](size_t b) { return frame_offsets[b + 1] - frame_offsets[b]; });
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // namespace

extern "C" {

int gvtm_synthesize_batch_host(gvtm_plan* plan, const float* params, const int32_t* frame_counts,
		size_t batch, size_t max_frames, float* audio, size_t audio_stride,
		int64_t* out_counts, float* maxabs)
{
	if (batch != 0 && !audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	return host_pipeline(plan, HostJob{params, frame_counts, nullptr, batch, max_frames, audio, nullptr, audio_stride, out_counts, maxabs, nullptr});
}

int gvtm_synthesize_voices_host(gvtm_plan* plan, const float* params, const int32_t* frame_counts, const int32_t* voice_ids,
		size_t max_frames, size_t batch, float* audio, size_t audio_stride, int64_t* out_counts, float* maxabs)
{
	if (batch != 0 && !audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if (batch != 0 && !voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null voice ids");
	return host_pipeline(plan, HostJob{params, frame_counts, voice_ids, batch, max_frames, audio, nullptr, audio_stride, out_counts, maxabs, nullptr});
}

int gvtm_synthesize_batch_host_pcm16(gvtm_plan* plan, const float* params, const int32_t* frame_counts,
		size_t batch, size_t max_frames, int16_t* pcm, size_t pcm_stride,
		int64_t* out_counts, float* maxabs, float* scales)
{
	if (batch != 0 && !pcm) return fail(GVTM_ERR_INVALID_ARGUMENT, "null pcm buffer");
	return host_pipeline(plan, HostJob{params, frame_counts, nullptr, batch, max_frames, nullptr, pcm, pcm_stride, out_counts, maxabs, scales});
}

int gvtm_synthesize_voices_host_pcm16(gvtm_plan* plan, const float* params, const int32_t* frame_counts, const int32_t* voice_ids,
		size_t max_frames, size_t batch, int16_t* pcm, size_t pcm_stride, int64_t* out_counts, float* maxabs, float* scales)
{
	if (batch != 0 && !pcm) return fail(GVTM_ERR_INVALID_ARGUMENT, "null pcm buffer");
	if (batch != 0 && !voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null voice ids");
	return host_pipeline(plan, HostJob{params, frame_counts, voice_ids, batch, max_frames, nullptr, pcm, pcm_stride, out_counts, maxabs, scales});
}

size_t gvtm_packed_sample_offsets(const gvtm_plan* plan, const int64_t* frame_offsets, const int32_t* voice_ids, size_t batch, int64_t* sample_offsets_out)
{
	try {
		std::vector<int64_t> offsets;
		if (packed_layout(plan, frame_offsets, voice_ids, batch, offsets) != GVTM_OK) return static_cast<size_t>(-1);
		if (sample_offsets_out) std::copy(offsets.begin(), offsets.end(), sample_offsets_out);
		return static_cast<size_t>(offsets[batch]);
	} catch (const std::bad_alloc&) {
		fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
		return static_cast<size_t>(-1);
	}
}

int gvtm_synthesize_packed_host(gvtm_plan* plan, const float* frames, const int64_t* frame_offsets, const int32_t* voice_ids, size_t batch,
		float* audio, size_t audio_capacity, int64_t* sample_offsets_out, int64_t* out_counts, float* maxabs)
{
	return packed_pipeline(plan, PackedJob{frames, frame_offsets, voice_ids, batch, {audio, nullptr, false, audio_capacity, sample_offsets_out, out_counts, maxabs, nullptr}});
}

int gvtm_synthesize_packed_host_pcm16(gvtm_plan* plan, const float* frames, const int64_t* frame_offsets, const int32_t* voice_ids, size_t batch,
		int16_t* pcm, size_t pcm_capacity, int64_t* sample_offsets_out, int64_t* out_counts, float* maxabs, float* scales)
{
	return packed_pipeline(plan, PackedJob{frames, frame_offsets, voice_ids, batch, {nullptr, pcm, true, pcm_capacity, sample_offsets_out, out_counts, maxabs, scales}});
}

size_t gvtm_events_packed_layout(const gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks,
		const int32_t* voice_ids, size_t batch, int64_t* frame_offsets_out, int64_t* sample_offsets_out)
{
	try {
		std::vector<int64_t> frame_offsets, offsets;
		if (events_packed_layout(plan, events, chunk_offsets, utt_chunks, voice_ids, batch, frame_offsets, offsets) != GVTM_OK) return static_cast<size_t>(-1);
		if (frame_offsets_out) std::copy(frame_offsets.begin(), frame_offsets.end(), frame_offsets_out);
		if (sample_offsets_out) std::copy(offsets.begin(), offsets.end(), sample_offsets_out);
		return static_cast<size_t>(offsets[batch]);
	} catch (const std::bad_alloc&) {
		fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
		return static_cast<size_t>(-1);
	}
}

int gvtm_synthesize_events_packed_host(gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks,
		const int32_t* voice_ids, size_t batch, float* audio, size_t audio_capacity, int64_t* sample_offsets_out, int64_t* frame_offsets_out,
		float* frames_out, size_t frames_capacity, int64_t* out_counts, float* maxabs, gvtm_drift_state* drift)
{
	return events_packed_pipeline(plan, EventsPackedJob{events, chunk_offsets, utt_chunks, voice_ids, batch,
			{audio, nullptr, false, audio_capacity, sample_offsets_out, out_counts, maxabs, nullptr}, frame_offsets_out, frames_out, frames_capacity, drift});
}

int gvtm_synthesize_events_packed_host_pcm16(gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks,
		const int32_t* voice_ids, size_t batch, int16_t* pcm, size_t pcm_capacity, int64_t* sample_offsets_out, int64_t* frame_offsets_out,
		float* frames_out, size_t frames_capacity, int64_t* out_counts, float* maxabs, float* scales, gvtm_drift_state* drift)
{
	return events_packed_pipeline(plan, EventsPackedJob{events, chunk_offsets, utt_chunks, voice_ids, batch,
			{nullptr, pcm, true, pcm_capacity, sample_offsets_out, out_counts, maxabs, scales}, frame_offsets_out, frames_out, frames_capacity, drift});
}

} // extern "C"
