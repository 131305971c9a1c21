// C ABI of libgama_vtm.so (see include/gama_vtm.h), the plan: status and last error, creation (design, device, table
// upload), queries, timing, the voices' track table, the staging limit and page-locked host memory.  No exception crosses
// the extern "C" frame (the reference's plugin convention: construct returns nullptr, VocalTractModelPlugin.cpp:87-90).
#include <cstring>
#include <memory>
#include <new>

#include "vtm_host.hpp"

namespace gvtm::host {

thread_local std::string g_last_error;

int fail(int status, const std::string& msg)
{
	g_last_error = msg;
	return status;
}

int fail_hip(hipError_t e, const char* what)
{
	return fail(GVTM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Is there a HIP device at this index?  (what: the caller, which has no CPU path)
int check_device_index(int device, const char* what)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(GVTM_ERR_NO_DEVICE, std::string("no HIP device available (") + what + " has no CPU path)");
	if (device < 0 || device >= n) return fail(GVTM_ERR_NO_DEVICE, "device index out of range");
	return GVTM_OK;
}

} // namespace gvtm::host

using namespace gvtm::host;

namespace {

// The device part of every plan: a HIP device at that index, a gfx950 one, and its compute units
int open_device(gvtm_plan* plan, int device)
{
	if (const int rc = check_device_index(device, "libgama_vtm"); rc != GVTM_OK) return rc;
	plan->device = device;
	hipDeviceProp_t prop;
	if (const hipError_t e = hipGetDeviceProperties(&prop, device); e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
	if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		return fail(GVTM_ERR_NO_DEVICE, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
	}
	plan->compute_units = prop.multiProcessorCount;
	return GVTM_OK;
}

// The device tables of a plan: one constants block per voice (model 5: one of each kind), back to back, and the
// converter's tables, which depend on no configuration key: voice 0's serve all.  The other models add one wavetable per
// voice and the glottal FIR (voice 0's, for the same reason).  A float plan (GVTM_PRECISION_F32, either model) uploads
// the tables as designed in float.
int upload_tables(gvtm_plan* plan)
{
	const gvtm::Design& dg = plan->designs[0];
	std::vector<gvtm::DeviceConstants> consts;
	std::vector<gvtm::Model5Constants> consts5;
	std::vector<double> wavetables;
	std::vector<float> wavetables_f;
	for (const gvtm::Design& dv : plan->designs) {
		consts.push_back(dv.k);
		if (dg.model5) consts5.push_back(dv.k5);
		wavetables.insert(wavetables.end(), dv.wavetable.begin(), dv.wavetable.end());
		wavetables_f.insert(wavetables_f.end(), dv.wavetable_f.begin(), dv.wavetable_f.end());
	}
	// the float or the double design of a table
	auto upload_design = [&](DeviceBuffer& dst, const std::vector<double>& wide, const std::vector<float>& narrow, const char* what) {
		return dg.f32 ? upload(dst, narrow, what) : upload(dst, wide, what);
	};
	int rc = GVTM_OK;
	if (!dg.model5) {
		if ((rc = upload_design(plan->d_wavetable, wavetables, wavetables_f, "upload wavetable")) != GVTM_OK) return rc;
		if ((rc = upload_design(plan->d_fir, dg.fir, dg.fir_f, "upload fir")) != GVTM_OK) return rc;
	}
	{
		// the targets' filter by voice, as gvtm_synthesize_targets_device forms the two for its one voice (vtm_capi_targets.cpp);
		// model 5 plans too: gvtm_synthesize_targets_model5_voices_device reads them
		std::vector<int64_t> targets_N;
		std::vector<double> targets_invN;
		for (const gvtm::Design& dv : plan->designs) {
			targets_N.push_back(gvtm::targets_filter_length(internal_rate_hz(dv)));
			targets_invN.push_back(1.0 / static_cast<double>(targets_N.back()));
		}
		if ((rc = upload(plan->d_targets_N, targets_N, "upload targets filter lengths")) != GVTM_OK) return rc;
		if ((rc = upload(plan->d_targets_invN, targets_invN, "upload targets filter reciprocals")) != GVTM_OK) return rc;
	}
	if ((rc = upload_design(plan->d_src_h, dg.src_h, dg.src_h_f, "upload src_h")) != GVTM_OK) return rc;
	if ((rc = upload_design(plan->d_src_dh, dg.src_dh, dg.src_dh_f, "upload src_dh")) != GVTM_OK) return rc;
	if ((rc = upload(plan->d_consts, consts, "upload constants")) != GVTM_OK) return rc;
	if (plan->src_phases) {
		// the converter's coefficients by output phase, once per plan; a plan that cannot have the memory does without
		const std::vector<float> table = gvtm::design_src_phase_table(dg);
		if (plan->d_src_phase.ensure(sizeof(float) * table.size()) != hipSuccess) {
			(void) hipGetLastError();
			plan->src_phases = 0;
		} else if (const hipError_t e = hipMemcpy(plan->d_src_phase.ptr, table.data(), sizeof(float) * table.size(), hipMemcpyHostToDevice); e != hipSuccess) {
			return fail_hip(e, "upload converter phase table");
		}
	}
	return dg.model5 ? upload(plan->d_consts5, consts5, "upload model 5 constants") : GVTM_OK;
}

// Every plan: `differs` refuses a voice that does not share `shared_keys` with voice 0, `design` designs each voice
// (gvtm_config: design_plan, gvtm5_config: design_plan5 or design_plan5_float), and upload_tables puts the tables on the device;
// float5_voices: the plan is gvtm_plan_create_model5_float_voices'
template <typename Config, typename Differs>
int create_plan(const Config* configs, size_t n_voices, double control_rate, int device, gvtm_plan** plan_out, const char* shared_keys,
		Differs differs, std::string (*design)(const Config&, double, gvtm::Design&), bool float5_voices = false)
{
	if (!configs || !plan_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null config or plan_out");
	*plan_out = nullptr;
	if (n_voices == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "a plan needs at least one voice");
	if (n_voices > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "too many voices");
	for (size_t v = 1; v < n_voices; ++v) {
		if (differs(configs[0], configs[v])) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, "voice " + std::to_string(v) + ": " + shared_keys + " must be those of voice 0 "
					"(one plan is one model at one output rate)");
		}
	}
	try {
		std::unique_ptr<gvtm_plan, void (*)(gvtm_plan*)> plan(new gvtm_plan, gvtm_plan_destroy);
		plan->designs.resize(n_voices);
		for (size_t v = 0; v < n_voices; ++v) {
			const std::string why = design(configs[v], control_rate, plan->designs[v]);
			if (!why.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, n_voices > 1 ? "voice " + std::to_string(v) + ": " + why : why);
		}
		plan->precision = configs[0].precision; // (model 5: the one precision the design of its class takes)
		plan->float5_voices = float5_voices;
		// the float decimator as this host's libm designs it against the table the float kernels hold as literals: a host
		// that designs another filter runs the generic tap loop over its own coefficients, and stays right
		const gvtm::Design& d0 = plan->designs[0];
		plan->fir_literals = !d0.model5 && d0.f32 && d0.fir_f.size() == static_cast<size_t>(gvtm::kGlottalFirTapsF32)
				&& std::memcmp(d0.fir_f.data(), gvtm::kGlottalFirF32, sizeof(gvtm::kGlottalFirF32)) == 0;
		// what is fixed for the plan and said once: the converter's coefficients by output phase and "the wavetable is
		// static".  One voice only: the voices of a plan have each their own internal rate and pulse shape, and the voice
		// variant of the kernel keeps forming both per pass
		if (n_voices == 1 && !d0.model5) {
			plan->src_phases = gvtm::src_phase_count(d0);
			plan->static_wavetable = gvtm::static_wavetable(d0.k);
		}
		if (device == GVTM_DEVICE_NONE) {
			// design-only plan: info, tables and output counts work, synthesis reports NO_DEVICE
			plan->device = GVTM_DEVICE_NONE;
			*plan_out = plan.release();
			return GVTM_OK;
		}
		int rc = open_device(plan.get(), device);
		if (rc != GVTM_OK) return rc;
		DeviceScope scope(device);
		if ((rc = scope.entered()) != GVTM_OK || (rc = upload_tables(plan.get())) != GVTM_OK) return rc;
		*plan_out = plan.release();
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	} catch (const std::exception& ex) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, ex.what());
	}
}

void fill_info(const gvtm_plan* plan, const gvtm::Design& dg, gvtm_info* info)
{
	const gvtm::DeviceConstants& k = dg.k;
	info->internal_sample_rate = k.sample_rate;
	info->control_steps = k.control_steps;
	info->output_rate = dg.config.output_rate;
	info->control_rate = dg.control_rate;
	info->fir_taps = k.fir_taps;
	info->time_register_increment = k.time_inc;
	info->phase_increment = k.phase_inc;
	info->pad_size = k.pad;
	info->upsampling = k.upsampling;
	info->device = plan->device;
	info->precision = plan->precision;
	info->section_delay = k.section_delay;
	info->model5 = dg.model5 ? 1 : 0;
	info->reserved_ = 0;
	info->internal_rate_hz = dg.model5 ? dg.k5.sample_rate : static_cast<double>(k.sample_rate);
}

} // namespace

extern "C" {

const char* gvtm_status_string(int status)
{
	switch (status) {
	case GVTM_OK: return "ok";
	case GVTM_ERR_INVALID_ARGUMENT: return "invalid argument";
	case GVTM_ERR_NO_DEVICE: return "no HIP device";
	case GVTM_ERR_HIP: return "HIP runtime error";
	case GVTM_ERR_UNSUPPORTED: return "unsupported";
	case GVTM_ERR_OUT_OF_MEMORY: return "out of memory";
	default: return "unknown status";
	}
}

const char* gvtm_last_error(void)
{
	return g_last_error.c_str();
}

int gvtm_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int gvtm_plan_create(const gvtm_config* config, double control_rate, int device, gvtm_plan** plan_out)
{
	return gvtm_plan_create_voices(config, 1, control_rate, device, plan_out);
}

int gvtm_plan_create_voices(const gvtm_config* configs, size_t n_voices, double control_rate, int device, gvtm_plan** plan_out)
{
	auto differs = [](const gvtm_config& c0, const gvtm_config& c) {
		return c.output_rate != c0.output_rate || c.section_delay != c0.section_delay || c.precision != c0.precision || c.tube_layout != c0.tube_layout;
	};
	return create_plan(configs, n_voices, control_rate, device, plan_out, "output_rate, section_delay, precision and tube_layout", differs,
			gvtm::design_plan);
}

int gvtm_plan_voice_count(const gvtm_plan* plan)
{
	if (!plan) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	return plan->n_voices();
}

int gvtm_plan_voice_info(const gvtm_plan* plan, int voice, gvtm_info* info)
{
	if (!plan || !info) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or info");
	if (voice < 0 || voice >= plan->n_voices()) return fail(GVTM_ERR_INVALID_ARGUMENT, "voice index out of range");
	fill_info(plan, plan->designs[voice], info);
	return GVTM_OK;
}

size_t gvtm_voice_output_count(const gvtm_plan* plan, int voice, size_t n_frames)
{
	if (!plan || voice < 0 || voice >= plan->n_voices()) return static_cast<size_t>(-1);
	return design_output_count(plan->designs[voice], n_frames);
}

size_t gvtm_voices_output_capacity(const gvtm_plan* plan, size_t max_frames)
{
	if (!plan) return static_cast<size_t>(-1);
	size_t m = 0;
	for (int v = 0; v < plan->n_voices(); ++v) m = std::max(m, design_output_capacity(plan->designs[v], max_frames));
	return m;
}

int gvtm_plan_create_model5(const gvtm5_config* config, double control_rate, int device, gvtm_plan** plan_out)
{
	return gvtm_plan_create_model5_voices(config, 1, control_rate, device, plan_out);
}

int gvtm_plan_create_model5_voices(const gvtm5_config* configs, size_t n_voices, double control_rate, int device, gvtm_plan** plan_out)
{
	auto differs = [](const gvtm5_config& c0, const gvtm5_config& c) { return c.output_rate != c0.output_rate || c.precision != c0.precision; };
	return create_plan(configs, n_voices, control_rate, device, plan_out, "output_rate and precision", differs, gvtm::design_plan5);
}

int gvtm_plan_create_model5_float(const gvtm5_config* config, double control_rate, int device, gvtm_plan** plan_out)
{
	auto differs = [](const gvtm5_config&, const gvtm5_config&) { return false; }; // (one voice)
	return create_plan(config, 1, control_rate, device, plan_out, "", differs, gvtm::design_plan5_float);
}

int gvtm_plan_create_model5_float_voices(const gvtm5_config* configs, size_t n_voices, double control_rate, int device, gvtm_plan** plan_out)
{
	auto differs = [](const gvtm5_config& c0, const gvtm5_config& c) { return c.output_rate != c0.output_rate || c.precision != c0.precision; };
	return create_plan(configs, n_voices, control_rate, device, plan_out, "output_rate and precision", differs, gvtm::design_plan5_float, true);
}

void gvtm_plan_destroy(gvtm_plan* plan)
{
	if (!plan) return;
	if (plan->device == GVTM_DEVICE_NONE) { // (a design-only plan holds nothing on a device)
		delete plan;
		return;
	}
	DeviceScope scope(plan->device);
	delete plan;
}

int gvtm_plan_info(const gvtm_plan* plan, gvtm_info* info)
{
	if (!plan || !info) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or info");
	fill_info(plan, plan->designs[0], info); // (a plan of several voices: voice 0)
	return GVTM_OK;
}

int gvtm_plan_table(const gvtm_plan* plan, int which, double* out, size_t capacity)
{
	if (!plan || !out) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or out");
	const std::vector<double>* src = nullptr;
	switch (which) {
	case GVTM_TABLE_FIR: src = &plan->designs[0].fir; break;
	case GVTM_TABLE_SRC_H: src = &plan->designs[0].src_h; break;
	case GVTM_TABLE_SRC_DH: src = &plan->designs[0].src_dh; break;
	case GVTM_TABLE_WAVETABLE: src = &plan->designs[0].wavetable; break;
	default: return -fail(GVTM_ERR_INVALID_ARGUMENT, "unknown table");
	}
	if (src->empty()) return -fail(GVTM_ERR_INVALID_ARGUMENT, "this model has no such table");
	if (capacity < src->size()) return -fail(GVTM_ERR_INVALID_ARGUMENT, "table buffer too small");
	std::memcpy(out, src->data(), sizeof(double) * src->size());
	return static_cast<int>(src->size());
}

size_t gvtm_output_count(const gvtm_plan* plan, size_t n_frames)
{
	if (!plan) return static_cast<size_t>(-1);
	return design_output_count(plan->designs[0], n_frames);
}

size_t gvtm_output_capacity(const gvtm_plan* plan, size_t max_frames)
{
	if (!plan) return static_cast<size_t>(-1);
	return design_output_capacity(plan->designs[0], max_frames);
}

int gvtm_plan_set_timing(gvtm_plan* plan, int enabled)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->timing = enabled != 0;
	return GVTM_OK;
}

double gvtm_plan_take_kernel_ms(gvtm_plan* plan, int* launches_out)
{
	if (launches_out) *launches_out = 0;
	if (!plan || plan->device == GVTM_DEVICE_NONE || plan->pending.empty()) return -1.0;
	DeviceScope scope(plan->device);
	double total = 0.0;
	int n = 0;
	for (EventPair& ev : plan->pending) {
		float ms = 0.f;
		if (hipEventSynchronize(ev.stop.h) == hipSuccess && hipEventElapsedTime(&ms, ev.start.h, ev.stop.h) == hipSuccess) {
			total += ms;
			++n;
		}
		plan->pool.push_back(std::move(ev));
	}
	plan->pending.clear();
	if (launches_out) *launches_out = n;
	return n ? total / n : -1.0;
}

int gvtm_plan_set_voice_tracks(gvtm_plan* plan, const gvtm_track_config* configs, size_t n_configs)
{
	if (!plan || !configs) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or configs");
	if (n_configs != static_cast<size_t>(plan->n_voices())) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, std::to_string(n_configs) + " track configurations for a plan of " + std::to_string(plan->n_voices()) + " voices");
	}
	try {
		// (the whole table is designed before any of it replaces the plan's: a refused call changes nothing)
		std::vector<gvtm::TrackConstants> table(n_configs);
		for (size_t v = 0; v < n_configs; ++v) {
			const std::string voice = "voice " + std::to_string(v) + ": ";
			const char* why = gvtm::design_tracks(configs[v], table[v]);
			if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, voice + why);
			if (!control_period_matches(plan, table[v])) {
				return fail(GVTM_ERR_INVALID_ARGUMENT, voice + "control_period_ms of the track configuration and the plan's control rate disagree");
			}
		}
		if (plan->device != GVTM_DEVICE_NONE) {
			DeviceScope scope(plan->device);
			if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
			// (the same size every time: the buffer is allocated once, and a call in flight must not see it rewritten)
			if (const int rc = upload(plan->d_voice_tracks, table, "upload voice track constants"); rc != GVTM_OK) return rc;
		}
		plan->voice_tracks = std::move(table);
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

int gvtm_host_alloc(size_t bytes, void** ptr_out)
{
	if (!ptr_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null ptr_out");
	*ptr_out = nullptr;
	if (bytes == 0) return GVTM_OK;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(GVTM_ERR_NO_DEVICE, "no HIP device available: page-locked memory comes from the HIP runtime");
	const hipError_t e = hipHostMalloc(ptr_out, bytes, hipHostMallocPortable);
	if (e != hipSuccess) { *ptr_out = nullptr; return e == hipErrorOutOfMemory ? fail(GVTM_ERR_OUT_OF_MEMORY, "hipHostMalloc: out of memory") : fail_hip(e, "hipHostMalloc"); }
	return GVTM_OK;
}

void gvtm_host_free(void* ptr)
{
	if (ptr) (void) hipHostFree(ptr);
}

int gvtm_plan_set_staging_limit(gvtm_plan* plan, size_t bytes)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->host.limit = bytes;
	// what an earlier call holds beyond the new limit goes now (every packed call drains its streams before it returns)
	if (bytes && plan->device != GVTM_DEVICE_NONE && plan->host.staging_bytes() > bytes) {
		DeviceScope scope(plan->device);
		if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
		plan->host.release_sets();
	}
	return GVTM_OK;
}

int gvtm_plan_packed_stats(const gvtm_plan* plan, gvtm_packed_stats* out)
{
	if (!plan || !out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or out");
	out->staging_bytes = plan->host.staging_bytes();
	out->limit = plan->host.limit;
	out->slices = plan->host.slices;
	out->largest_slice = plan->host.largest_slice;
	return GVTM_OK;
}

} // extern "C"
