// C ABI of libgama_vtm.so, streams: the stateful form of the path (include/gama_vtm.h, "Streams"), fed frames or
// event lists or parameter targets.
#include <cstring>
#include <memory>
#include <new>

#include "vtm_host.hpp"
#include "vtm_targets.hpp"

using namespace gvtm::host;

enum StreamFeed : int { kFeedNone = 0, kFeedFrames = 1, kFeedEvents = 2, kFeedTargets = 3 };

// the points of one parameter of one utterance of a targets-fed run, in absolute steps
struct TargetsLog {
	std::vector<int32_t> steps;
	std::vector<float> values;
};

struct gvtm_stream {
	gvtm_plan* plan = nullptr;
	size_t batch = 0;
	size_t state_stride = 0;              // the largest of the plan's voices (reset_voices never reallocates)
	int xr = 0;                           // ring length: the longest of the plan's voices (each voice keeps its own in the kernel)
	std::vector<unsigned> granule_frames; // per voice of the plan: pushes are synthesized in multiples of this many frames
	// a plan of several voices (gvtm_stream_create_voices): utterance b is spoken by voice_ids[b], a copy of which is on the
	// device for the grouping kernel
	bool voices = false;
	std::vector<int32_t> voice_ids;
	DeviceBuffer d_state, d_params, d_frames, d_audio, d_counts, d_maxabs, d_voice_ids, d_groups;
	std::vector<std::vector<float>> held; // per utterance: frames pushed but not yet synthesized (the last one is the look-ahead)
	std::vector<uint64_t> steps_done;     // per utterance: internal steps synthesized
	std::vector<float> staging;
	std::vector<int32_t> counts;
	bool finished = false;
	// how the stream has been fed since the last reset: frames (gvtm_stream_push), event lists (gvtm_stream_push_events) or
	// parameter targets (gvtm_stream_push_targets, model 5: gvtm_stream_push_targets_model5); one way per run
	int feed = kFeedNone;
	// a targets-fed run: utterance b's parameter p keeps in tg_log[16 b + p] the points the rule still needs in front of the
	// utterance's next step (vtm_targets.hpp: targets_first_needed) -- every launch uploads them all, and they are few: those
	// of the filter's window and of the pending steps, and one more -- and tg_pending[b] steps are pushed but not yet
	// synthesized (fewer than tg_granule after a push).  The filters' sums are in the device state.
	std::vector<TargetsLog> tg_log;
	std::vector<uint64_t> tg_pending;
	int64_t tg_N = 0;
	// a targets-fed run synthesizes in multiples of this many steps and keeps the rest: the steps at which the serial
	// wavefronts' states are exact (create_stream: 12; model 5: 4)
	uint64_t tg_granule = 0;
	DeviceBuffer d_tg_offsets, d_tg_steps, d_tg_values;
	// an events-fed run keeps its unsynthesized frames on the device: utterance b's in the rows [0, held_rows[b]) of its block
	// of held_cap rows of d_held ([batch][held_cap][16]; at least one row of a block stays spare: a push's launch reads
	// max_frames - 1 rows at most).  The tracks kernel appends behind them, the synthesis launch reads them in place, the
	// carry kernel moves what the launch left to the front.
	DeviceBuffer d_held;
	size_t held_cap = 0;
	std::vector<size_t> held_rows;
	// the drift generators, one per utterance (fresh at create; no reset touches them), and the tables of a push: events,
	// the two offset tables, {row_start, rows held} [2][batch] and the frames the tracks kernel counted
	DeviceBuffer d_drift, d_events, d_chunk_offsets, d_utt_chunks, d_rows, d_new_counts;
};

namespace {

unsigned gcd_u(unsigned a, unsigned b)
{
	while (b) { const unsigned t = a % b; a = b; b = t; }
	return a;
}

int voice_of(const gvtm_stream* s, size_t b)
{
	return s->voices ? s->voice_ids[b] : 0;
}

int stream_upload_fresh_state(gvtm_stream* s)
{
	std::vector<unsigned char> init(s->state_stride * s->batch, 0);
	const bool model5 = s->plan->designs[0].model5;
	for (size_t b = 0; b < s->batch; ++b) {
		gvtm::StreamHeader h{};
		h.seed = 0.7892347; // NoiseSource::reset (vtm/NoiseSource.h:32-34)
		std::memcpy(init.data() + b * s->state_stride, &h, sizeof(h));
		if (model5) {
			// VocalTractModel5::reset (vtm/VocalTractModel5.h:423-453): RosenbergBGlottalSource::reset leaves t2 at the end of the
			// longest falling phase, the noise source starts from its seed, everything else is zero
			const gvtm::Model5Constants& k5 = s->plan->designs[voice_of(s, b)].k5;
			double sc[gvtm::kStream5Scalars] = {};
			// (the float class adds in float)
			sc[gvtm::kS5Scan + 1] = s->plan->designs[0].f32 ? static_cast<double>(static_cast<float>(k5.rb_t1) + static_cast<float>(k5.rb_tn_max))
			                                                : k5.rb_t1 + k5.rb_tn_max;
			sc[gvtm::kS5Scan + 2] = 0.7892347;
			std::memcpy(init.data() + b * s->state_stride + gvtm::Stream5Layout::scalars(), sc, sizeof(sc));
		}
	}
	return upload(s->d_state, init, "upload stream state"); // (the same size every time: allocated at create)
}

// the stream's drift generators from host states, or (null) fresh ones (DriftGenerator.cpp:28, :40)
int stream_upload_drift(gvtm_stream* s, const gvtm_drift_state* states)
{
	std::vector<gvtm_drift_state> fresh;
	if (!states) {
		fresh.assign(s->batch, gvtm_drift_state{0.7892347, 0.0, 0.0, 0.0, 0.0});
		states = fresh.data();
	}
	return upload(s->d_drift, states, s->batch, "upload drift states");
}

uint64_t outputs_before(const gvtm::DeviceConstants& k, uint64_t steps)
{
	return ((steps << 16) + k.time_inc - 1) / k.time_inc;
}

// the internal steps of n of what the stream is fed: frames, or in a targets-fed run steps
uint64_t feed_steps(const gvtm_stream* s, size_t b, size_t n)
{
	return s->feed == kFeedTargets ? static_cast<uint64_t>(n) : static_cast<uint64_t>(n) * s->plan->designs[voice_of(s, b)].k.control_steps;
}

// The samples of one launch on behalf of the stream, known before it: utterance b synthesizes n_frames[b] more frames (a
// targets-fed run: steps).
// want[b]: its exact sample count; need: the largest of them; too_long: an utterance would pass the 2^31-step limit.
struct StreamSamples {
	std::vector<int64_t> want;
	size_t need = 0;
	bool too_long = false;
};

StreamSamples stream_samples(const gvtm_stream* s, const std::vector<size_t>& n_frames, bool final)
{
	StreamSamples r{std::vector<int64_t>(s->batch, 0)};
	for (size_t b = 0; b < s->batch; ++b) {
		const gvtm::DeviceConstants& k = s->plan->designs[voice_of(s, b)].k;
		const uint64_t after = s->steps_done[b] + feed_steps(s, b, n_frames[b]);
		if (after + 4096ull >= (1ull << 31)) r.too_long = true;
		const uint64_t k1 = final ? gvtm::src_output_count(k.time_inc, k.pad, k.upsampling, after) : outputs_before(k, after);
		r.want[b] = static_cast<int64_t>(k1 - outputs_before(k, s->steps_done[b]));
		r.need = std::max(r.need, static_cast<size_t>(r.want[b]));
	}
	return r;
}

// the most steps a targets-fed run keeps pending after a push, whatever the plan: one short of the largest granule
// (gvtm_stream::tg_granule), which gvtm_stream_targets_capacity counts on
constexpr uint64_t kTargetsMostPending = 11;
constexpr int32_t kTargetsNullTables = -1;

// One utterance of a gvtm_stream_push_targets or gvtm_stream_push_targets_model5 call, `count` steps of at most max_steps with the 17 offsets `off`: the status
// of gvtm_targets_apply_host in its order, where a point at or beyond `count` is a bad step too (4); kTargetsNullTables for
// points without their tables.
int32_t targets_push_status(const int64_t* off, const int32_t* point_steps, const float* point_values, int64_t count, int64_t max_steps)
{
	if (count < 0 || count > max_steps) return gvtm::kTargetsBadCount;
	for (int p = 0; p < GVTM_N_PARAM; ++p) {
		if (off[p] < 0 || off[p + 1] < off[p]) return gvtm::kTargetsBadOffsets;
	}
	if (off[GVTM_N_PARAM] > off[0] && (!point_steps || !point_values)) return kTargetsNullTables;
	for (int64_t j = off[0]; j < off[GVTM_N_PARAM]; ++j) {
		if (!gvtm::modification_finite(point_values[j])) return gvtm::kTargetsBadValue;
	}
	for (int p = 0; p < GVTM_N_PARAM; ++p) {
		for (int64_t j = off[p]; j < off[p + 1]; ++j) {
			if (gvtm::targets_bad_step(point_steps, off[p], j) || point_steps[j] >= count) return gvtm::kTargetsBadSteps;
		}
	}
	return gvtm::kTargetsOk;
}

// forget what the rule no longer needs in front of step s0
void targets_forget(TargetsLog& log, int64_t s0, int64_t N)
{
	const int64_t keep = gvtm::targets_first_needed(log.steps.data(), 0, static_cast<int64_t>(log.steps.size()), N, s0);
	log.steps.erase(log.steps.begin(), log.steps.begin() + keep);
	log.values.erase(log.values.begin(), log.values.begin() + keep);
}

// The log of a targets-fed run as the tables of a targets launch: list 16 b + p holds utterance b's parameter p, the points
// back to back.  (No table is empty on the device: the launch takes no null pointer.)
int stream_upload_targets(gvtm_stream* s)
{
	std::vector<int64_t> offsets(s->tg_log.size() + 1, 0);
	for (size_t l = 0; l < s->tg_log.size(); ++l) offsets[l + 1] = offsets[l] + static_cast<int64_t>(s->tg_log[l].steps.size());
	std::vector<int32_t> steps(static_cast<size_t>(offsets.back()));
	std::vector<float> values(steps.size());
	for (size_t l = 0; l < s->tg_log.size(); ++l) {
		std::copy(s->tg_log[l].steps.begin(), s->tg_log[l].steps.end(), steps.begin() + offsets[l]);
		std::copy(s->tg_log[l].values.begin(), s->tg_log[l].values.end(), values.begin() + offsets[l]);
	}
	int rc = upload(s->d_tg_offsets, offsets, "upload target list offsets");
	if (rc == GVTM_OK) rc = upload(s->d_tg_steps, steps.data(), steps.size(), "upload target steps", 1);
	if (rc == GVTM_OK) rc = upload(s->d_tg_values, values.data(), values.size(), "upload target values", 1);
	return rc;
}

// One launch on behalf of the stream: utterance b synthesizes n_frames[b] frames from the front of held[b] -- or, in an
// events-fed run, from the front of its block of d_held, which the launch reads in place (no staging, no copy of frames);
// behind a push's launch the carry kernel then moves the rows it left to the front of the block.  In a targets-fed run
// n_frames counts steps, there are no frames, and the launch walks the stream's log of points (stream_upload_targets).
int stream_launch(gvtm_stream* s, const std::vector<size_t>& n_frames, bool final, float* audio, size_t audio_stride, int64_t* out_counts,
		float* maxabs, bool* launched = nullptr)
{
	gvtm_plan* plan = s->plan;
	const size_t batch = s->batch;
	const bool targets = s->feed == kFeedTargets;
	const size_t ahead = final || targets ? 0 : 1; // a push of frames carries the look-ahead frame behind its last one
	size_t rows_max = 0;
	bool lockstep = true, any = final;
	// (lockstep is judged per voice: a workgroup only ever holds one voice; first[v] is voice v's first utterance)
	std::vector<size_t> first(static_cast<size_t>(plan->n_voices()), batch);
	for (size_t b = 0; b < batch; ++b) {
		const size_t rows = n_frames[b] + ahead;
		rows_max = std::max(rows_max, n_frames[b] ? rows : size_t(0));
		size_t& f = first[static_cast<size_t>(voice_of(s, b))];
		if (f == batch) f = b;
		if (n_frames[b] != n_frames[f] || s->steps_done[b] != s->steps_done[f]) lockstep = false;
		if (n_frames[b]) any = true;
	}
	const StreamSamples samples = stream_samples(s, n_frames, final);
	if (samples.too_long) return fail(GVTM_ERR_INVALID_ARGUMENT, "a stream holds at most 2^31 internal steps between resets");
	if (samples.need > audio_stride) return fail(GVTM_ERR_INVALID_ARGUMENT, "audio_stride smaller than this call produces (gvtm_stream_capacity)");
	if (samples.need > 0 && !audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if (!any) {
		if (out_counts) std::fill(out_counts, out_counts + batch, int64_t(0));
		return GVTM_OK;
	}
	const bool on_device = s->feed == kFeedEvents;
	if (on_device) rows_max = s->held_cap; // (the row stride of d_held: every block has a row behind the frames a push synthesizes)
	if (rows_max == 0) rows_max = 1;
	DeviceScope scope(plan->device);
	int rc = scope.entered();
	if (rc != GVTM_OK) return rc;
	hipError_t e;
	const bool staged = !on_device && !targets; // frames from host memory
	try {
		s->staging.assign(staged ? batch * rows_max * GVTM_N_PARAM : 0, 0.0f);
		s->counts.assign(batch, 0);
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
	for (size_t b = 0; b < batch; ++b) {
		if (!n_frames[b]) continue;
		const size_t rows = n_frames[b] + ahead;
		if (staged) std::memcpy(s->staging.data() + b * rows_max * GVTM_N_PARAM, s->held[b].data(), sizeof(float) * rows * GVTM_N_PARAM);
		s->counts[b] = static_cast<int32_t>(n_frames[b]);
	}
	const size_t abytes = sizeof(float) * batch * std::max<size_t>(audio_stride, 1);
	if (staged && (rc = upload(s->d_params, s->staging, "upload params")) != GVTM_OK) return rc;
	if (targets && (rc = stream_upload_targets(s)) != GVTM_OK) return rc;
	if ((rc = upload(s->d_frames, s->counts, "upload frame counts")) != GVTM_OK) return rc;
	if ((e = s->d_audio.ensure(abytes)) != hipSuccess) return fail_hip(e, "hipMalloc audio");
	if ((e = s->d_counts.ensure(sizeof(int64_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc counts");
	if ((e = s->d_maxabs.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc maxabs");
	if ((e = hipMemsetAsync(s->d_audio.ptr, 0, abytes, nullptr)) != hipSuccess) return fail_hip(e, "hipMemsetAsync");
	const StreamLaunch sl{static_cast<unsigned char*>(s->d_state.ptr), s->state_stride, final ? gvtm::kStreamFinish : gvtm::kStreamPush, s->xr};
	// (one utterance per workgroup unless the utterances are in lockstep)
	float* const d_rows_in = targets ? nullptr : on_device ? s->d_held.as<float>() : s->d_params.as<float>();
	LaunchRequest request{d_rows_in, s->d_frames.as<int32_t>(), batch, rows_max, s->d_audio.as<float>(), audio_stride, s->d_counts.as<int64_t>(),
			s->d_maxabs.as<float>(), nullptr, lockstep ? 0 : 1, s->voices, s->voices ? s->d_voice_ids.as<int32_t>() : nullptr, &s->d_groups, &sl};
	const TargetsLaunch tl{s->d_tg_offsets.as<int64_t>(), nullptr, s->d_tg_steps.as<int32_t>(), s->d_tg_values.as<float>(), s->tg_N,
			1.0 / static_cast<double>(std::max<int64_t>(s->tg_N, 1))};
	if (targets) request.targets = &tl;
	rc = launch_synthesis(plan, request);
	if (rc != GVTM_OK) return rc;
	if (launched) *launched = true;
	if (on_device && !final) {
		// (d_rows: the rows each block held when the launch began, behind the row starts of the push)
		const gvtm::CarryArgs ca{d_rows_in, s->d_frames.as<int32_t>(), s->d_rows.as<int32_t>() + batch, batch, rows_max};
		if ((e = gvtm::launch_carry_rows(ca, nullptr)) != hipSuccess) return fail_hip(e, "vtm_carry_rows_kernel launch");
	}
	if ((e = hipDeviceSynchronize()) != hipSuccess) return fail_hip(e, "vtm_synth_kernel execution");
	std::vector<int64_t> got(batch, 0);
	if ((rc = download(got.data(), s->d_counts, batch, "D2H counts")) != GVTM_OK) return rc;
	for (size_t b = 0; b < batch; ++b) {
		if (got[b] != samples.want[b]) return fail(GVTM_ERR_HIP, "internal error: the device's sample count differs from the host's");
	}
	if (audio && (rc = download(audio, s->d_audio, batch * audio_stride, "D2H audio")) != GVTM_OK) return rc;
	if (out_counts) std::copy(got.begin(), got.end(), out_counts);
	if (maxabs && (rc = download(maxabs, s->d_maxabs, batch, "D2H maxabs")) != GVTM_OK) return rc;
	for (size_t b = 0; b < batch; ++b) {
		s->steps_done[b] += feed_steps(s, b, n_frames[b]);
		if (targets) s->tg_pending[b] -= n_frames[b];
		else if (on_device) s->held_rows[b] -= n_frames[b];
		else s->held[b].erase(s->held[b].begin(), s->held[b].begin() + static_cast<std::ptrdiff_t>(n_frames[b] * GVTM_N_PARAM));
	}
	return GVTM_OK;
}

// gvtm_stream_create (voice_ids null) and gvtm_stream_create_voices on a plan of several voices.  The state stride and
// the ring are sized for the largest voice of the plan, whichever voices the ids name, so that gvtm_stream_reset_voices
// never reallocates.
int create_stream(gvtm_plan* plan, size_t batch, const int32_t* voice_ids, gvtm_stream** stream_out)
{
	try {
		std::unique_ptr<gvtm_stream, void (*)(gvtm_stream*)> s(new gvtm_stream, gvtm_stream_destroy);
		s->plan = plan;
		s->batch = batch;
		s->voices = voice_ids != nullptr;
		if (s->voices) s->voice_ids.assign(voice_ids, voice_ids + batch);
		if (!plan->designs[0].model5) s->xr = plan->longest_stream_ring();
		for (int v = 0; v < plan->n_voices(); ++v) {
			const gvtm::DeviceConstants& k = plan->designs[v].k;
			if (plan->designs[0].model5) {
				// reference model 5: its own state block (vtm_kernels.hpp: Stream5Layout); the serial wavefronts work in blocks
				// of four steps (vtm_kernel_m5.inc)
				s->state_stride = gvtm::Stream5Layout::bytes();
				s->granule_frames.push_back(4u / gcd_u(k.control_steps, 4u));
				s->tg_granule = 4; // (a targets-fed run, gvtm_stream_push_targets_model5: the same blocks of four)
			} else {
				// each voice's ring is the one-row shape's, whatever shape a launch takes (the kernel derives it per voice)
				const int xr = plan->stream_ring(v);
				s->state_stride = std::max(s->state_stride, gvtm::stream_state_bytes(k, plan->precision, xr));
				// the serial wavefronts work in blocks of 2, 4 and 4 or 6 steps (vtm_kernel_v2.inc): their states are exact at
				// multiples of 12 steps, so a push synthesizes a multiple of 12 / gcd(control_steps, 12) frames and keeps the rest
				s->granule_frames.push_back(12u / gcd_u(k.control_steps, 12u));
				s->tg_granule = 12;
			}
		}
		s->held.resize(batch);
		s->held_rows.assign(batch, 0);
		s->steps_done.assign(batch, 0);
		s->tg_log.resize(batch * GVTM_N_PARAM);
		s->tg_pending.assign(batch, 0);
		s->tg_N = gvtm::targets_filter_length(internal_rate_hz(plan->designs[0]));
		DeviceScope scope(plan->device);
		int rc = scope.entered();
		// (one voice: every utterance's id is 0, which only the tracks kernel of an events-fed run reads)
		if (rc == GVTM_OK) rc = upload_voice_ids(s->d_voice_ids, voice_ids, batch);
		if (rc == GVTM_OK) rc = stream_upload_fresh_state(s.get());
		if (rc == GVTM_OK) rc = stream_upload_drift(s.get(), nullptr);
		if (rc != GVTM_OK) return rc;
		*stream_out = s.release();
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

// the most rows a block of d_held may have: launch_synthesis takes the row stride as max_frames, whose steps must fit its
// 31-bit step counter
size_t stream_block_limit(const gvtm_plan* plan)
{
	return static_cast<size_t>(((1ull << 31) - 4096ull - 1ull) / std::max(1u, max_control_steps(plan)));
}

// What gvtm_stream_push_events does once its checks have passed: have[b] rows held after the push, fresh[b] of them new,
// n[b] of them synthesized by it.  Up to the tracks launch a failure leaves the stream as it was; from there on
// (*advanced) its drift generators have moved.
int stream_append_and_launch(gvtm_stream* s, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks, size_t n_chunks,
		size_t n_events, const std::vector<size_t>& fresh, const std::vector<size_t>& have, const std::vector<size_t>& n, float* audio,
		size_t audio_stride, int64_t* out_counts, bool* advanced)
{
	gvtm_plan* plan = s->plan;
	const size_t batch = s->batch;
	DeviceScope scope(plan->device);
	int rc = scope.entered();
	if (rc != GVTM_OK) return rc;
	hipError_t e;
	// the blocks of d_held: the rows held and one spare.  A larger buffer is a new one, the rows held copied over device to
	// device (DeviceBuffer::ensure would free them first)
	const size_t need_cap = *std::max_element(have.begin(), have.end()) + 1;
	if (need_cap > s->held_cap) {
		// (half as much again, within what a launch takes as max_frames)
		const size_t new_cap = std::max(need_cap, std::min(s->held_cap + s->held_cap / 2, stream_block_limit(plan)));
		const size_t kept = *std::max_element(s->held_rows.begin(), s->held_rows.end());
		constexpr size_t row_bytes = sizeof(float) * GVTM_N_PARAM;
		DeviceBuffer grown;
		if ((e = grown.ensure(row_bytes * batch * new_cap)) != hipSuccess) return fail_hip(e, "hipMalloc held frames");
		if (kept && (e = hipMemcpy2D(grown.ptr, row_bytes * new_cap, s->d_held.ptr, row_bytes * s->held_cap, row_bytes * kept, batch,
				hipMemcpyDeviceToDevice)) != hipSuccess) return fail_hip(e, "D2D held frames");
		s->d_held = std::move(grown); // (the old buffer goes with `grown`)
		s->held_cap = new_cap;
	}
	// the tables of the push, one copy each into buffers of the stream's
	std::vector<int64_t> no_chunks;
	std::vector<int32_t> rows(2 * batch);
	for (size_t b = 0; b < batch; ++b) {
		rows[b] = static_cast<int32_t>(s->held_rows[b]);
		rows[batch + b] = static_cast<int32_t>(have[b]);
	}
	if (!utt_chunks) {
		no_chunks.assign(batch + 1, 0);
		utt_chunks = no_chunks.data();
	}
	const int64_t zero = 0;
	if (n_chunks == 0) chunk_offsets = &zero;
	// (the events' pointer goes to the kernel even when there are none)
	if ((rc = upload(s->d_events, events, n_events, "upload events", 1)) != GVTM_OK) return rc;
	if ((rc = upload(s->d_chunk_offsets, chunk_offsets, n_chunks + 1, "upload chunk offsets")) != GVTM_OK) return rc;
	if ((rc = upload(s->d_utt_chunks, utt_chunks, batch + 1, "upload utterance chunks")) != GVTM_OK) return rc;
	if ((rc = upload(s->d_rows, rows, "upload row starts")) != GVTM_OK) return rc;
	if ((e = s->d_new_counts.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frame counts");
	// append, synthesis, carry: all on the stream's launch stream
	gvtm::TrackAppendArgs ta = plan_track_args(plan, s->d_events.as<gvtm_event>(), s->d_voice_ids.as<int32_t>(), batch, s->held_cap, s->d_held.as<float>(),
			s->d_new_counts.as<int32_t>(), s->d_drift.as<gvtm_drift_state>());
	ta.chunk_offsets = s->d_chunk_offsets.as<int64_t>();
	ta.utt_chunks = s->d_utt_chunks.as<int64_t>();
	ta.row_start = s->d_rows.as<int32_t>();
	if ((e = gvtm::launch_tracks(ta, nullptr)) != hipSuccess) return fail_hip(e, "track generation launch (append)");
	*advanced = true;
	s->feed = kFeedEvents;
	s->held_rows = have;
	if ((rc = stream_launch(s, n, false, audio, audio_stride, out_counts, nullptr)) != GVTM_OK) return rc;
	// (a push that synthesizes nothing launches nothing behind the tracks kernel: the copy waits for it)
	return check_device_frame_counts(s->d_new_counts, batch, [&](size_t b) { return fresh[b]; });
}

// What gvtm_stream_push_targets and gvtm_stream_push_targets_model5 share, which is everything behind the choice of plans:
// the refusals in their order, the status pass, the roll-back, the log, targets_forget and the launch.  The granule is the
// stream's (tg_granule).
int stream_push_targets(gvtm_stream* s, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values,
		const int32_t* step_counts, size_t max_steps, float* audio, size_t audio_stride, int64_t* out_counts, int32_t* status_out)
{
	if (s->finished) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream has been finished: gvtm_stream_reset() starts the next utterances");
	if (s->feed == kFeedFrames) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream is fed frames (gvtm_stream_push) until the next gvtm_stream_reset()");
	if (s->feed == kFeedEvents) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream is fed event lists (gvtm_stream_push_events) until the next gvtm_stream_reset()");
	if (!list_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null list_offsets");
	if (!gvtm::targets_fits_step_counter(static_cast<int64_t>(std::min<size_t>(max_steps, INT64_MAX)))) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "max_steps does not fit the 31-bit step counter");
	}
	const size_t batch = s->batch;
	// every utterance's status first: a refused one refuses the call, and nothing has been touched
	size_t refused = batch;
	for (size_t b = 0; b < batch; ++b) {
		const int64_t count = step_counts ? static_cast<int64_t>(step_counts[b]) : static_cast<int64_t>(max_steps);
		const int32_t status = targets_push_status(list_offsets + b * GVTM_N_PARAM, point_steps, point_values, count, static_cast<int64_t>(max_steps));
		if (status == kTargetsNullTables) return fail(GVTM_ERR_INVALID_ARGUMENT, "null point_steps or point_values with points");
		if (status_out) status_out[b] = status;
		if (status != gvtm::kTargetsOk && refused == batch) refused = b;
	}
	if (refused < batch) return fail(GVTM_ERR_INVALID_ARGUMENT, "utterance " + std::to_string(refused) + " is refused (status_out says why); nothing was pushed");
	for (size_t b = 0; b < batch; ++b) {
		const uint64_t count = step_counts ? static_cast<uint64_t>(step_counts[b]) : static_cast<uint64_t>(max_steps);
		if (s->steps_done[b] + s->tg_pending[b] + count + 4096ull >= (1ull << 31)) return fail(GVTM_ERR_INVALID_ARGUMENT, "a stream holds at most 2^31 internal steps between resets");
	}
	// a call that fails before its launch leaves the stream as it found it: the points and steps it appended are taken back
	const int feed_before = s->feed;
	const std::vector<uint64_t> pending_before = s->tg_pending;
	std::vector<size_t> held_before(s->tg_log.size(), 0);
	for (size_t l = 0; l < s->tg_log.size(); ++l) held_before[l] = s->tg_log[l].steps.size();
	auto roll_back = [&]() {
		for (size_t l = 0; l < s->tg_log.size(); ++l) {
			s->tg_log[l].steps.resize(held_before[l]);
			s->tg_log[l].values.resize(held_before[l]);
		}
		s->tg_pending = pending_before;
		s->feed = feed_before;
	};
	try {
		std::vector<size_t> n(batch, 0);
		for (size_t b = 0; b < batch; ++b) {
			// the push's step 0 is the first step the utterance has not been given yet
			const int64_t base = static_cast<int64_t>(s->steps_done[b] + s->tg_pending[b]);
			for (int p = 0; p < GVTM_N_PARAM; ++p) {
				TargetsLog& log = s->tg_log[b * GVTM_N_PARAM + p];
				for (int64_t j = list_offsets[b * GVTM_N_PARAM + p]; j < list_offsets[b * GVTM_N_PARAM + p + 1]; ++j) {
					log.steps.push_back(static_cast<int32_t>(base + point_steps[j]));
					log.values.push_back(point_values[j]);
				}
			}
			s->tg_pending[b] += step_counts ? static_cast<uint64_t>(step_counts[b]) : static_cast<uint64_t>(max_steps);
			// the serial wavefronts' states are exact at multiples of the granule (create_stream); no step waits for a successor
			n[b] = static_cast<size_t>(s->tg_pending[b] / s->tg_granule * s->tg_granule);
		}
		s->feed = kFeedTargets;
		bool launched = false;
		const int rc = stream_launch(s, n, false, audio, audio_stride, out_counts, nullptr, &launched);
		if (rc != GVTM_OK && !launched) roll_back(); // (after the launch the device state has moved on: gvtm_stream_reset is the way out)
		if (rc == GVTM_OK) {
			for (size_t b = 0; b < batch; ++b) {
				for (int p = 0; p < GVTM_N_PARAM; ++p) targets_forget(s->tg_log[b * GVTM_N_PARAM + p], static_cast<int64_t>(s->steps_done[b]), s->tg_N);
			}
		}
		return rc;
	} catch (const std::bad_alloc&) {
		roll_back();
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // namespace

extern "C" {

int gvtm_stream_create(gvtm_plan* plan, size_t batch, gvtm_stream** stream_out)
{
	if (!plan || !stream_out || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan / stream_out or empty batch");
	*stream_out = nullptr;
	if (plan->n_voices() > 1) return refuse_voices(plan, "gvtm_stream_create");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	return create_stream(plan, batch, nullptr, stream_out);
}

int gvtm_stream_create_voices(gvtm_plan* plan, const int32_t* voice_ids, size_t batch, gvtm_stream** stream_out)
{
	if (stream_out) *stream_out = nullptr;
	if (!plan || !stream_out || !voice_ids || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan / stream_out / voice_ids or empty batch");
	if (const int rc = check_voice_ids(plan, voice_ids, batch); rc != GVTM_OK) return rc;
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	// (a plan of one voice: every id is 0, and the stream is the one gvtm_stream_create makes)
	return create_stream(plan, batch, plan->n_voices() > 1 ? voice_ids : nullptr, stream_out);
}

void gvtm_stream_destroy(gvtm_stream* s)
{
	if (!s) return;
	DeviceScope scope(s->plan->device);
	delete s;
}

int gvtm_stream_reset(gvtm_stream* s)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	DeviceScope scope(s->plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	for (auto& h : s->held) h.clear();
	std::fill(s->held_rows.begin(), s->held_rows.end(), size_t(0));
	std::fill(s->steps_done.begin(), s->steps_done.end(), uint64_t(0));
	// (a targets-fed run's sums go with the fresh state: an utterance at step 0 begins its filters anew)
	for (TargetsLog& l : s->tg_log) l = TargetsLog();
	std::fill(s->tg_pending.begin(), s->tg_pending.end(), uint64_t(0));
	s->finished = false;
	s->feed = kFeedNone; // (the drift generators run on: the reference's Controller never reseeds its own)
	return stream_upload_fresh_state(s);
}

int gvtm_stream_reset_voices(gvtm_stream* s, const int32_t* voice_ids)
{
	if (!s || !voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream or voice_ids");
	int rc = check_voice_ids(s->plan, voice_ids, s->batch);
	if (rc != GVTM_OK) return rc;
	// past the checks the stream takes the new ids; a device error from here on leaves it finished (pushes refused) until a
	// reset succeeds, so that no push runs on half-reset state
	if (s->voices) {
		std::copy(voice_ids, voice_ids + s->batch, s->voice_ids.begin());
		DeviceScope scope(s->plan->device);
		// (the buffer holds batch ids since create: no reallocation)
		if ((rc = scope.entered()) == GVTM_OK) rc = upload_voice_ids(s->d_voice_ids, voice_ids, s->batch);
	}
	if (rc == GVTM_OK) rc = gvtm_stream_reset(s);
	if (rc != GVTM_OK) s->finished = true;
	return rc;
}

size_t gvtm_stream_capacity(const gvtm_stream* s, size_t max_new_frames)
{
	if (!s) return static_cast<size_t>(-1);
	// the largest over the stream's voices: at most the new frames plus what a push can have kept (the voice's granule),
	// flushed, with the overrun's lap
	size_t m = 0;
	for (int v = 0; v < s->plan->n_voices(); ++v) {
		if (s->voices && std::find(s->voice_ids.begin(), s->voice_ids.end(), v) == s->voice_ids.end()) continue;
		const gvtm::DeviceConstants& k = s->plan->designs[v].k;
		const uint64_t steps = static_cast<uint64_t>(max_new_frames + s->granule_frames[static_cast<size_t>(v)]) * k.control_steps;
		m = std::max(m, static_cast<size_t>(gvtm::src_output_capacity(k.time_inc, k.pad, k.upsampling, steps) + 1));
	}
	return m;
}

int gvtm_stream_push(gvtm_stream* s, const float* params, const int32_t* frame_counts, size_t max_frames,
		float* audio, size_t audio_stride, int64_t* out_counts)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->finished) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream has been finished: gvtm_stream_reset() starts the next utterances");
	if (s->feed == kFeedEvents) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream is fed event lists (gvtm_stream_push_events) until the next gvtm_stream_reset()");
	if (s->feed == kFeedTargets) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream is fed targets (gvtm_stream_push_targets, model 5: gvtm_stream_push_targets_model5) until the next gvtm_stream_reset()");
	if (max_frames > 0 && !params) return fail(GVTM_ERR_INVALID_ARGUMENT, "null params with max_frames > 0");
	if (frame_counts) {
		for (size_t b = 0; b < s->batch; ++b) {
			if (frame_counts[b] < 0 || static_cast<size_t>(frame_counts[b]) > max_frames) return fail(GVTM_ERR_INVALID_ARGUMENT, "frame_counts entry outside [0, max_frames]");
		}
	}
	// a call that fails (a stride too small, a null buffer, an allocation) leaves the stream as it found it: the frames it
	// appended are taken back, so that the corrected call does not synthesize them twice
	std::vector<size_t> held_before(s->batch, 0);
	for (size_t b = 0; b < s->batch; ++b) held_before[b] = s->held[b].size();
	auto roll_back = [&]() {
		for (size_t b = 0; b < s->batch; ++b) {
			if (s->held[b].size() > held_before[b]) s->held[b].resize(held_before[b]);
		}
	};
	try {
		std::vector<size_t> n(s->batch, 0);
		for (size_t b = 0; b < s->batch; ++b) {
			const size_t add = frame_counts ? static_cast<size_t>(frame_counts[b]) : max_frames;
			const float* src = params + b * max_frames * GVTM_N_PARAM;
			s->held[b].insert(s->held[b].end(), src, src + add * GVTM_N_PARAM);
			const size_t have = s->held[b].size() / GVTM_N_PARAM;
			// the last frame held is the look-ahead of the one before it (Controller.cpp:297-300 interpolates towards the NEXT frame)
			const unsigned granule = s->granule_frames[static_cast<size_t>(voice_of(s, b))];
			n[b] = have > 0 ? ((have - 1) / granule) * granule : 0;
		}
		bool launched = false;
		const int rc = stream_launch(s, n, false, audio, audio_stride, out_counts, nullptr, &launched);
		if (rc != GVTM_OK && !launched) roll_back(); // (after the launch the device state has moved on: gvtm_stream_reset is the way out)
		else s->feed = kFeedFrames;
		return rc;
	} catch (const std::bad_alloc&) {
		roll_back();
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

int gvtm_stream_finish(gvtm_stream* s, float* audio, size_t audio_stride, int64_t* out_counts, float* maxabs)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->finished) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream has already been finished");
	try {
		std::vector<size_t> n(s->batch, 0);
		// the last frame stands for its own successor (Controller.cpp:283); a targets-fed run: the pending steps
		for (size_t b = 0; b < s->batch; ++b) {
			n[b] = s->feed == kFeedTargets ? static_cast<size_t>(s->tg_pending[b]) : s->feed == kFeedEvents ? s->held_rows[b] : s->held[b].size() / GVTM_N_PARAM;
		}
		const int rc = stream_launch(s, n, true, audio, audio_stride, out_counts, maxabs);
		if (rc == GVTM_OK) s->finished = true;
		return rc;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

size_t gvtm_stream_targets_capacity(const gvtm_stream* s, size_t max_new_steps)
{
	if (!s) return static_cast<size_t>(-1);
	// the new steps and what a push can have kept (one short of the largest granule: model 5 keeps 3 at most), flushed, with
	// the overrun's lap
	const gvtm::DeviceConstants& k = s->plan->designs[0].k;
	return static_cast<size_t>(gvtm::src_output_capacity(k.time_inc, k.pad, k.upsampling, static_cast<uint64_t>(max_new_steps) + kTargetsMostPending) + 1);
}

int gvtm_stream_targets_points(const gvtm_stream* s, int64_t* held_out)
{
	if (!s || !held_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream or held_out");
	for (size_t b = 0; b < s->batch; ++b) {
		held_out[b] = 0;
		for (int p = 0; p < GVTM_N_PARAM; ++p) held_out[b] += static_cast<int64_t>(s->tg_log[b * GVTM_N_PARAM + p].steps.size());
	}
	return GVTM_OK;
}

int gvtm_stream_push_targets(gvtm_stream* s, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values,
		const int32_t* step_counts, size_t max_steps, float* audio, size_t audio_stride, int64_t* out_counts, int32_t* status_out)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->plan->n_voices() > 1) return fail(GVTM_ERR_UNSUPPORTED, "gvtm_stream_push_targets: a plan of one voice only");
	if (s->plan->designs[0].model5) return fail(GVTM_ERR_UNSUPPORTED, "gvtm_stream_push_targets: the models 0 to 4 only");
	return stream_push_targets(s, list_offsets, point_steps, point_values, step_counts, max_steps, audio, audio_stride, out_counts, status_out);
}

int gvtm_stream_push_targets_model5(gvtm_stream* s, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values,
		const int32_t* step_counts, size_t max_steps, float* audio, size_t audio_stride, int64_t* out_counts, int32_t* status_out)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->plan->n_voices() > 1) return fail(GVTM_ERR_UNSUPPORTED, "gvtm_stream_push_targets_model5: a plan of one voice only (the models 0 to 4: gvtm_stream_push_targets)");
	if (!s->plan->designs[0].model5) return fail(GVTM_ERR_UNSUPPORTED, "gvtm_stream_push_targets_model5: model 5 only; the models 0 to 4 have gvtm_stream_push_targets");
	return stream_push_targets(s, list_offsets, point_steps, point_values, step_counts, max_steps, audio, audio_stride, out_counts, status_out);
}

int gvtm_stream_push_events(gvtm_stream* s, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks, float* audio,
		size_t audio_stride, int64_t* out_counts, int32_t* frame_counts_out)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->finished) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream has been finished: gvtm_stream_reset() starts the next utterances");
	if (s->feed == kFeedFrames) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream is fed frames (gvtm_stream_push) until the next gvtm_stream_reset()");
	if (s->feed == kFeedTargets) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream is fed targets (gvtm_stream_push_targets, model 5: gvtm_stream_push_targets_model5) until the next gvtm_stream_reset()");
	const gvtm_plan* plan = s->plan;
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, "gvtm_stream_push_events: the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	const size_t batch = s->batch;
	// (a null utt_chunks: no utterance receives a chunk)
	const int64_t last_chunk = utt_chunks ? utt_chunks[batch] : 0;
	if (last_chunk > 0 && (!events || !chunk_offsets)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events or chunk_offsets");
	if (utt_chunks && check_offsets(utt_chunks, batch, "utt_chunks", FirstOffset::kNotNegative) != GVTM_OK) return GVTM_ERR_INVALID_ARGUMENT;
	const size_t n_chunks = last_chunk > 0 ? static_cast<size_t>(last_chunk) : 0;
	if (check_offsets(chunk_offsets, n_chunks, "chunk_offsets", FirstOffset::kNotBelowZero) != GVTM_OK) return GVTM_ERR_INVALID_ARGUMENT;
	const size_t n_events = n_chunks ? static_cast<size_t>(chunk_offsets[n_chunks]) : 0;
	try {
		// what the tracks kernel will generate, counted here: every sample count is known before anything is launched
		const int cp = plan->voice_tracks[0].control_period; // (every voice's is the plan's: gvtm_plan_set_voice_tracks)
		std::vector<size_t> fresh(batch, 0), have(batch, 0), n(batch, 0);
		for (size_t b = 0; b < batch; ++b) {
			if (utt_chunks) fresh[b] = chunks_frame_count(cp, events, chunk_offsets, utt_chunks[b], utt_chunks[b + 1]);
			have[b] = s->held_rows[b] + fresh[b];
			// (the rows of a block, the spare one included, are the synthesis launch's max_frames)
			if (have[b] + 1 > stream_block_limit(plan)) return fail(GVTM_ERR_INVALID_ARGUMENT, "utterance " + std::to_string(b) + ": too many frames for one push");
			// as gvtm_stream_push: the last frame held is the look-ahead of the one before it
			const unsigned granule = s->granule_frames[static_cast<size_t>(voice_of(s, b))];
			n[b] = have[b] > 0 ? ((have[b] - 1) / granule) * granule : 0;
		}
		const StreamSamples samples = stream_samples(s, n, false);
		if (samples.need > audio_stride) return fail(GVTM_ERR_INVALID_ARGUMENT, "audio_stride smaller than this call produces (gvtm_stream_capacity)");
		if (samples.need > 0 && !audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
		if (samples.too_long) return fail(GVTM_ERR_INVALID_ARGUMENT, "a stream holds at most 2^31 internal steps between resets");
		bool advanced = false;
		const int rc = stream_append_and_launch(s, events, chunk_offsets, utt_chunks, n_chunks, n_events, fresh, have, n, audio, audio_stride, out_counts, &advanced);
		// past the tracks launch the drift generators and the held frames have moved on: no push until a reset
		if (rc != GVTM_OK && advanced) s->finished = true;
		if (rc == GVTM_OK && frame_counts_out) {
			for (size_t b = 0; b < batch; ++b) frame_counts_out[b] = static_cast<int32_t>(fresh[b]);
		}
		return rc;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

int gvtm_stream_get_drift(const gvtm_stream* s, gvtm_drift_state* states_out)
{
	if (!s || !states_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream or states_out");
	DeviceScope scope(s->plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	return download(states_out, s->d_drift, s->batch, "D2H drift states");
}

int gvtm_stream_set_drift(gvtm_stream* s, const gvtm_drift_state* states)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->feed == kFeedEvents) return fail(GVTM_ERR_INVALID_ARGUMENT, "the drift generators are running: gvtm_stream_reset() comes first");
	try {
		DeviceScope scope(s->plan->device);
		if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
		return stream_upload_drift(s, states);
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // extern "C"
