// C ABI of libgama_vtm.so, event lists from posture sequences: the compiled articulatory model (checked, copied, uploaded),
// the rule on the host, the rule for a batch on the device, and the postures entry, which puts those kernels in front of
// gvtm_synthesize_events_device with an event buffer of the plan's in between.
#include <memory>

#include "vtm_host.hpp"
#include "vtm_rules.hpp"

using namespace gvtm::host;

// The model as gvtm_rules_create took it: host copies behind `host`, and on a device the same arrays behind `device`
struct gvtm_rules {
	int device = GVTM_DEVICE_NONE;
	std::vector<float> floats;     // the model's float arrays, one after the other
	std::vector<int32_t> ints;     // ... its int32 arrays
	std::vector<uint8_t> bytes;    // ... the match table
	gvtm_rules_model host{};
	DeviceBuffer d_floats, d_ints, d_bytes;
	gvtm_rules_model on_device{};
};

namespace {

// the arrays of a model and their lengths, by element type, in one fixed order
struct ModelLayout {
	struct FloatArray { const float* gvtm_rules_model::*field; size_t count; };
	struct IntArray { const int32_t* gvtm_rules_model::*field; size_t count; };
	std::vector<FloatArray> floats;
	std::vector<IntArray> ints;
	size_t match_bytes;
	explicit ModelLayout(const gvtm_rules_model& m)
	{
		const size_t P = m.n_postures, R = m.n_rules;
		floats = {{&gvtm_rules_model::param_target, P * 16}, {&gvtm_rules_model::symbol_target, P * 6}, {&gvtm_rules_model::param_min, 16},
				{&gvtm_rules_model::param_max, 16}, {&gvtm_rules_model::program_const, static_cast<size_t>(m.n_program_ops)},
				{&gvtm_rules_model::point_value, static_cast<size_t>(m.n_points)}, {&gvtm_rules_model::point_free_time, static_cast<size_t>(m.n_points)},
				{&gvtm_rules_model::slopes, static_cast<size_t>(m.n_slopes)}};
		ints = {{&gvtm_rules_model::rule_n_expr, R}, {&gvtm_rules_model::rule_equations, R * 5}, {&gvtm_rules_model::rule_param_transition, R * 16},
				{&gvtm_rules_model::rule_special_transition, R * 16}, {&gvtm_rules_model::equation_offsets, static_cast<size_t>(m.n_equations) + 1},
				{&gvtm_rules_model::program_op, static_cast<size_t>(m.n_program_ops)}, {&gvtm_rules_model::transition_offsets, static_cast<size_t>(m.n_transitions) + 1},
				{&gvtm_rules_model::items, static_cast<size_t>(m.n_items) * 5}, {&gvtm_rules_model::point_type, static_cast<size_t>(m.n_points)},
				{&gvtm_rules_model::point_time_eq, static_cast<size_t>(m.n_points)}};
		match_bytes = R * 4 * P;
	}
};

// `to`: the counts of `from`, its arrays repointed into the three pools at the places `layout` gives them
void repoint(const ModelLayout& layout, const gvtm_rules_model& from, const float* floats, const int32_t* ints, const uint8_t* bytes, gvtm_rules_model& to)
{
	to = from;
	size_t at = 0;
	for (const auto& a : layout.floats) {
		to.*(a.field) = floats + at;
		at += a.count;
	}
	at = 0;
	for (const auto& a : layout.ints) {
		to.*(a.field) = ints + at;
		at += a.count;
	}
	to.match = bytes;
}

bool bad_control_period(int32_t cp) { return cp < 1 || cp > 4; }

} // namespace

int gvtm::host::rules_device(const gvtm_rules* rules) { return rules->device; }

extern "C" {

int gvtm_rules_create(int device, const gvtm_rules_model* model, gvtm_rules** rules_out)
{
	if (!model || !rules_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null model or rules_out");
	*rules_out = nullptr;
	const char* why = gvtm::rules_validate(*model);
	if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, std::string("rules model: ") + why);
	if (device != GVTM_DEVICE_NONE) {
		if (const int rc = check_device_index(device, "event generation"); rc != GVTM_OK) return rc;
	}
	auto rules = std::make_unique<gvtm_rules>();
	rules->device = device;
	const ModelLayout layout(*model);
	for (const auto& a : layout.floats) rules->floats.insert(rules->floats.end(), model->*(a.field), model->*(a.field) + a.count);
	for (const auto& a : layout.ints) rules->ints.insert(rules->ints.end(), model->*(a.field), model->*(a.field) + a.count);
	rules->bytes.assign(model->match, model->match + layout.match_bytes);
	repoint(layout, *model, rules->floats.data(), rules->ints.data(), rules->bytes.data(), rules->host);
	if (device != GVTM_DEVICE_NONE) {
		DeviceScope scope(device);
		int rc = scope.entered();
		// (a pool's pointer goes to the kernels even when it holds nothing)
		if (rc == GVTM_OK) rc = upload(rules->d_floats, rules->floats.data(), rules->floats.size(), "upload rules model (floats)", 1);
		if (rc == GVTM_OK) rc = upload(rules->d_ints, rules->ints.data(), rules->ints.size(), "upload rules model (ints)", 1);
		if (rc == GVTM_OK) rc = upload(rules->d_bytes, rules->bytes.data(), rules->bytes.size(), "upload rules model (match table)", 1);
		if (rc != GVTM_OK) return rc;
		repoint(layout, *model, rules->d_floats.as<float>(), rules->d_ints.as<int32_t>(), rules->d_bytes.as<uint8_t>(), rules->on_device);
	}
	*rules_out = rules.release();
	return GVTM_OK;
}

void gvtm_rules_destroy(gvtm_rules* rules)
{
	if (!rules) return;
	if (rules->device != GVTM_DEVICE_NONE) {
		DeviceScope scope(rules->device); // (hipFree of the pools on their device)
		delete rules;
		return;
	}
	delete rules;
}

int gvtm_rules_apply_host(const gvtm_rules* rules, int32_t control_period, const gvtm_posture* postures, size_t n, gvtm_event* events_out, size_t capacity,
		size_t* n_events_out, gvtm_rule_data* rule_data_out, size_t rule_capacity, size_t* n_rules_out, double* onsets_out, int32_t* status_out)
{
	if (!rules || !n_events_out || !status_out || (!postures && n > 0)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null rules, postures, n_events_out or status_out");
	if (bad_control_period(control_period)) return fail(GVTM_ERR_INVALID_ARGUMENT, "control_period must be 1..4");
	const int64_t events = gvtm::rules_apply(rules->host, control_period, postures, n, events_out, capacity, rule_data_out, rule_capacity, n_rules_out, onsets_out,
			status_out);
	*n_events_out = static_cast<size_t>(events);
	if (events_out && static_cast<size_t>(events) > capacity) return fail(GVTM_ERR_INVALID_ARGUMENT, "the event list does not fit capacity (gvtm_rules_event_count)");
	return GVTM_OK;
}

int64_t gvtm_rules_event_count(const gvtm_rules* rules, int32_t control_period, const gvtm_posture* postures, size_t n, int32_t* status_out)
{
	if (!rules || (!postures && n > 0)) { fail(GVTM_ERR_INVALID_ARGUMENT, "null rules or postures"); return -1; }
	if (bad_control_period(control_period)) { fail(GVTM_ERR_INVALID_ARGUMENT, "control_period must be 1..4"); return -1; }
	int32_t status = 0;
	const int64_t events = gvtm::rules_apply(rules->host, control_period, postures, n, nullptr, 0, nullptr, 0, nullptr, nullptr, &status);
	if (status_out) *status_out = status;
	return events;
}

int gvtm_generate_events_device(const gvtm_rules* rules, int32_t control_period, const gvtm_posture* d_postures, const int64_t* d_posture_offsets, size_t batch,
		gvtm_event* d_events_out, size_t out_capacity, int64_t* d_event_offsets_out, gvtm_rule_data* d_rule_data, size_t max_rules, int32_t* d_rule_counts,
		double* d_onsets, int32_t* d_status, void* hip_stream)
{
	if (!rules) return fail(GVTM_ERR_INVALID_ARGUMENT, "null rules");
	if (batch > 0 && (!d_postures || !d_posture_offsets || !d_events_out || !d_event_offsets_out)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null postures, posture offsets, events_out or event_offsets_out");
	}
	if (bad_control_period(control_period)) return fail(GVTM_ERR_INVALID_ARGUMENT, "control_period must be 1..4");
	if (batch > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	if (rules->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "rules created with GVTM_DEVICE_NONE: host use only");
	if (batch == 0) return GVTM_OK;
	DeviceScope scope(rules->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	gvtm::RulesArgs args{};
	args.m = rules->on_device;
	args.control_period = control_period;
	args.postures = d_postures;
	args.posture_offsets = d_posture_offsets;
	args.batch = batch;
	args.events_out = d_events_out;
	args.out_capacity = static_cast<int64_t>(std::min<size_t>(out_capacity, INT64_MAX));
	args.event_offsets_out = d_event_offsets_out;
	args.rule_data = d_rule_data;
	args.max_rules = d_rule_data ? static_cast<int64_t>(std::min<size_t>(max_rules, INT64_MAX)) : 0;
	args.rule_counts = d_rule_counts;
	args.onsets = d_onsets;
	args.status = d_status;
	const hipError_t e = gvtm::launch_generate_events(args, static_cast<hipStream_t>(hip_stream));
	return e == hipSuccess ? GVTM_OK : fail_hip(e, "event generation launch");
}

int gvtm_synthesize_postures_device(gvtm_plan* plan, const gvtm_rules* rules, const gvtm_track_config* config, const gvtm_posture* d_postures,
		const int64_t* d_posture_offsets, size_t events_capacity, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts,
		int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, int32_t* d_status, void* hip_stream)
{
	if (!plan || !config || !rules) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan, config or rules");
	if (plan->n_voices() > 1) return refuse_voices(plan, "gvtm_synthesize_postures_device");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (rules->device != plan->device) return fail(GVTM_ERR_INVALID_ARGUMENT, "the rules live on another device than the plan");
	if (batch == 0) return GVTM_OK;
	if (!d_postures || !d_posture_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null postures or posture offsets");
	// (what the synthesis entry would refuse is refused before the rule kernels write a status)
	gvtm::TrackConstants tk{};
	const char* why = gvtm::design_tracks(*config, tk);
	if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, why);
	if (!control_period_matches(plan, tk)) return fail(GVTM_ERR_INVALID_ARGUMENT, "control_period_ms of the track configuration and the plan's control rate disagree");
	if (!d_audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	int rc = check_audio_stride(plan, audio_stride, max_frames, false);
	if (rc != GVTM_OK) return rc;
	if (events_capacity > SIZE_MAX / sizeof(gvtm_event)) return fail(GVTM_ERR_INVALID_ARGUMENT, "events_capacity too large");
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	hipError_t e;
	// (the events' pointer goes to the kernels even when there is room for none)
	if ((e = plan->async.events.ensure(sizeof(gvtm_event) * std::max<size_t>(events_capacity, 1))) != hipSuccess) return fail_hip(e, "hipMalloc generated events");
	if ((e = plan->async.event_offsets.ensure(sizeof(int64_t) * (batch + 1))) != hipSuccess) return fail_hip(e, "hipMalloc generated event offsets");
	gvtm_event* events = plan->async.events.as<gvtm_event>();
	int64_t* offsets = plan->async.event_offsets.as<int64_t>();
	rc = gvtm_generate_events_device(rules, tk.control_period, d_postures, d_posture_offsets, batch, events, events_capacity, offsets, nullptr, 0, nullptr, nullptr,
			d_status, hip_stream);
	if (rc != GVTM_OK) return rc;
	return gvtm_synthesize_events_device(plan, config, events, offsets, batch, max_frames, d_audio, audio_stride, d_frame_counts, d_out_counts, d_maxabs, d_drift,
			hip_stream);
}

} // extern "C"
