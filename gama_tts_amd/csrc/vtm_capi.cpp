// C ABI of libgama_vtm.so (see include/gama_vtm.h).  Host side only: validation, table
// design/upload, launches.  No exception crosses the extern "C" frame (the reference's
// plugin convention: construct returns nullptr, VocalTractModelPlugin.cpp:87-90).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gama_vtm.h"
#include "vtm_design.hpp"
#include "vtm_kernels.hpp"
#include "vtm_pack.hpp"
#include "vtm_tracks.hpp"
#include "vtm_math.hpp"

namespace {

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
	hipError_t status() const { return status_; }
private:
	int previous_ = -1;
	bool changed_ = false;
	hipError_t status_ = hipSuccess;
};

} // namespace

#ifndef GVTM_NOISE_TABLE
#define GVTM_NOISE_TABLE 1
#endif

struct gvtm_plan {
	// one design per voice, voice 0 first (gvtm_plan_create_voices: several); d_consts, d_consts5 and d_wavetable hold one
	// block per voice, the FIR and the converter's tables (the same for every voice) one
	std::vector<gvtm::Design> designs;
	int device = 0;
	int precision = GVTM_PRECISION_F64;
	int rows = 0;       // utterances per workgroup; 0 = by batch size (a diagnostics build can force it)
	bool float5_voices = false; // made by gvtm_plan_create_model5_float_voices: a float model 5 plan that takes the voices entries
	// design tables on the device: double, or float (as designed) for GVTM_PRECISION_F32
	DeviceBuffer d_wavetable, d_fir, d_src_h, d_src_dh;
	DeviceBuffer d_consts, d_consts5; // gvtm::DeviceConstants, gvtm::Model5Constants (model 5 plans only)
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
	} host;
	// ... and the enqueue-only entries' (gvtm_synthesize_events_device's frames and frame counts, the grouping of
	// gvtm_synthesize_voices_device): calls to those on one plan must be ordered on one stream
	struct {
		DeviceBuffer params, frames, groups;
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
	std::vector<EventPair> pending;
	std::vector<EventPair> pool;
	// host-buffer entries: frames in on one stream, kernels on a second, samples out on a third (created on first use)
	Stream h2d_stream, compute_stream, copy_stream;
	std::vector<Event> slice_events; // three per slice: input arrived, output ready, output copied (recorded where sets rotate)

	int n_voices() const { return static_cast<int>(designs.size()); }
	// the shape of a launch of `batch` utterances (vtm_kernels.hpp: synth_launch_shape; forced_rows 0: the plan's own)
	gvtm::LaunchShape launch_shape(size_t batch, int forced_rows, bool voices, int stream_ring = 0, bool fit = true) const
	{
		return gvtm::synth_launch_shape(designs.data(), n_voices(), precision, batch, forced_rows ? forced_rows : rows, voices, stream_ring, fit);
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
	// voices launches the voice variant (gvtm_stream_create_voices)
	gvtm::LaunchShape stream_launch_shape(size_t batch, int forced_rows, int xr) const { return launch_shape(batch, forced_rows, n_voices() > 1, xr); }
};

namespace {

template <typename T>
hipError_t upload(DeviceBuffer& dst, const std::vector<T>& src)
{
	hipError_t e = dst.ensure(sizeof(T) * src.size());
	if (e != hipSuccess) return e;
	return hipMemcpy(dst.ptr, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
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

} // extern "C"

namespace {

// Is there a HIP device at this index?  (what: the caller, which has no CPU path)
int check_device_index(int device, const char* what)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(GVTM_ERR_NO_DEVICE, std::string("no HIP device available (") + what + " has no CPU path)");
	if (device < 0 || device >= n) return fail(GVTM_ERR_NO_DEVICE, "device index out of range");
	return GVTM_OK;
}

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
	auto upload_design = [&](DeviceBuffer& dst, const std::vector<double>& wide, const std::vector<float>& narrow) {
		return dg.f32 ? upload(dst, narrow) : upload(dst, wide);
	};
	hipError_t e;
	if (!dg.model5) {
		if ((e = upload_design(plan->d_wavetable, wavetables, wavetables_f)) != hipSuccess) return fail_hip(e, "upload wavetable");
		if ((e = upload_design(plan->d_fir, dg.fir, dg.fir_f)) != hipSuccess) return fail_hip(e, "upload fir");
	}
	if ((e = upload_design(plan->d_src_h, dg.src_h, dg.src_h_f)) != hipSuccess) return fail_hip(e, "upload src_h");
	if ((e = upload_design(plan->d_src_dh, dg.src_dh, dg.src_dh_f)) != hipSuccess) return fail_hip(e, "upload src_dh");
	if ((e = upload(plan->d_consts, consts)) != hipSuccess) return fail_hip(e, "upload constants");
	if (dg.model5 && (e = upload(plan->d_consts5, consts5)) != hipSuccess) return fail_hip(e, "upload model 5 constants");
	return GVTM_OK;
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
		if (device == GVTM_DEVICE_NONE) {
			// design-only plan: info, tables and output counts work, synthesis reports NO_DEVICE
			plan->device = GVTM_DEVICE_NONE;
			*plan_out = plan.release();
			return GVTM_OK;
		}
		int rc = open_device(plan.get(), device);
		if (rc != GVTM_OK) return rc;
		DeviceScope scope(device);
		hipError_t e = scope.status();
		if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
		if ((rc = upload_tables(plan.get())) != GVTM_OK) return rc;
		*plan_out = plan.release();
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	} catch (const std::exception& ex) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, ex.what());
	}
}

// The single-voice entry points on a plan of several voices: which voice would they synthesize?
int refuse_voices(const gvtm_plan* plan, const char* entry)
{
	return fail(GVTM_ERR_INVALID_ARGUMENT, std::string(entry) + ": the plan has " + std::to_string(plan->n_voices()) +
			" voices; use gvtm_synthesize_voices_* resp. gvtm_synthesize_events_voices_device (one voice id per utterance)");
}

// Everything that launches a kernel, on a design-only plan
int refuse_design_only()
{
	return fail(GVTM_ERR_NO_DEVICE, "design-only plan (GVTM_DEVICE_NONE): there is no CPU synthesis path");
}

// the most steps per frame among the plan's voices: what a launch is judged by, and what the noise table is as long as
unsigned max_control_steps(const gvtm_plan* plan)
{
	unsigned max_steps = 0;
	for (int v = 0; v < plan->n_voices(); ++v) max_steps = std::max(max_steps, plan->designs[v].k.control_steps);
	return max_steps;
}

// do utterances of `frames` frames fit the kernels' 31-bit step counter?
bool fits_step_counter(const gvtm_plan* plan, unsigned long long frames)
{
	return frames < (1ull << 31) && frames * max_control_steps(plan) + 4096ull < (1ull << 31);
}

// does the track configuration's control period agree with the plan's control rate?
bool control_period_matches(const gvtm_plan* plan, const gvtm::TrackConstants& tk)
{
	return static_cast<double>(tk.control_period) * plan->designs[0].control_rate == 1000.0;
}

// Track arguments for a batch of a plan of voices: from the plan its table on the device and the control period, which is
// every voice's (gvtm_plan_set_voice_tracks); the kernel variant's offset tables (and row_start) are the caller's to add
gvtm::TrackAppendArgs plan_track_args(const gvtm_plan* plan, const gvtm_event* d_events, const int32_t* d_voice_ids, size_t batch, size_t max_frames,
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

size_t design_output_count(const gvtm::Design& dg, size_t n_frames)
{
	const gvtm::DeviceConstants& k = dg.k;
	return static_cast<size_t>(gvtm::src_output_count(k.time_inc, k.pad, k.upsampling, static_cast<uint64_t>(n_frames) * k.control_steps));
}

size_t design_output_capacity(const gvtm::Design& dg, size_t max_frames)
{
	const gvtm::DeviceConstants& k = dg.k;
	return static_cast<size_t>(gvtm::src_output_capacity(k.time_inc, k.pad, k.upsampling, static_cast<uint64_t>(max_frames) * k.control_steps));
}

} // namespace

extern "C" {

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

#ifdef GVTM_DIAGNOSTICS
/* ---- hooks of the diagnostics build (libgama_vtm_diag.so; tests and tools only, not in the public header) ---- */
#pragma GCC visibility push(default)

/* Forces the utterances per workgroup (1, 2, 4, 8; 0 = by batch size), i.e. the kernel shape a big batch would get. */
int gvtm_debug_set_rows(gvtm_plan* plan, int rows)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->rows = rows;
	return GVTM_OK;
}

/* LDS bytes of a workgroup of `rows` utterances of this plan's one-shot kernel (0 = model 5's). */
size_t gvtm_debug_lds_bytes(const gvtm_plan* plan, int rows)
{
	if (!plan) return 0;
	// (of these rows, whether they fit or not; rows no launch has answer as the shape a launch forced to them has)
	return gvtm::synth_launch_shape(plan->designs.data(), 1, plan->precision, 0, rows, false, 0, false).lds;
}

/* The shape a launch of `batch` utterances of this plan takes (voices != 0: a gvtm_synthesize_voices_* launch), as
   launch_synthesis asks for it: out = {rows, ring length, LDS bytes}.  Needs no device. */
int gvtm_debug_launch_shape(const gvtm_plan* plan, size_t batch, int voices, size_t out[3])
{
	if (!plan || !out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or buffer");
	const gvtm::LaunchShape shape = plan->launch_shape(batch, 0, voices != 0);
	if (!shape.rows) return fail(GVTM_ERR_UNSUPPORTED, "LDS budget exceeded");
	out[0] = static_cast<size_t>(shape.rows), out[1] = static_cast<size_t>(shape.ring), out[2] = shape.lds;
	return GVTM_OK;
}

/* The same for a launch of a stream (not model 5) whose `batch` utterances are pushed in lockstep, which is how they
   share workgroups: the stream keeps the one-row shape's ring for every shape, so rows that fit a one-shot launch may
   not fit here and give way to half as many.  A plan of several voices answers for a gvtm_stream_create_voices stream:
   the voice variant, its LDS sized for the longest of the voices' stream rings. */
int gvtm_debug_stream_launch_shape(const gvtm_plan* plan, size_t batch, size_t out[3])
{
	if (!plan || !out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or buffer");
	if (plan->designs[0].model5) return fail(GVTM_ERR_UNSUPPORTED, "a plan of the models 0 to 4");
	const gvtm::LaunchShape shape = plan->stream_launch_shape(batch, 0, plan->longest_stream_ring());
	if (!shape.rows) return fail(GVTM_ERR_UNSUPPORTED, "LDS budget exceeded");
	out[0] = static_cast<size_t>(shape.rows), out[1] = static_cast<size_t>(shape.ring), out[2] = shape.lds;
	return GVTM_OK;
}

/* The chunk length (internal steps per tick) of the kernel shape a one-shot launch of `batch` utterances of this plan
   takes: synth_chunk_length of the rows launch_synthesis picks.  0: no shape (model 5, or none fits); negative: a null
   plan.  Needs no device. */
int gvtm_debug_chunk_length(const gvtm_plan* plan, size_t batch)
{
	if (!plan) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->designs[0].model5) return 0;
	const gvtm::LaunchShape shape = plan->launch_shape(batch, 0, false);
	if (!shape.rows) return 0;
	return gvtm::synth_chunk_length(plan->designs[0].k, plan->precision, shape.rows);
}

/* The plan-level noise-sample table as the host builds it (n floats or doubles); needs no device. */
int gvtm_debug_noise_table(size_t n, int as_float, void* out)
{
	if (!out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null buffer");
	gvtm::design_noise_table(n, as_float != 0, out);
	return GVTM_OK;
}

/* Test hook (not in the public header): device buffer [batch][max_frames*control_steps][8] of
 * doubles that receives per-step intermediate values of the next synthesis calls; null disables. */
int gvtm_debug_set_taps(gvtm_plan* plan, double* d_taps)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->debug_taps = d_taps;
	return GVTM_OK;
}

/* Diagnostic hook (not in the public header): device buffer [batch][16] of uint64 receiving the
 * shader cycles workgroup `b` spent per phase (generation 1) or per role wavefront [0..7] and per
 * helper stage [8..13] (generation 2). */
int gvtm_debug_set_phase_cycles(gvtm_plan* plan, unsigned long long* d_cycles)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->phase_cycles = d_cycles;
	return GVTM_OK;
}

/* Diagnostic hook: what each lane receives through the cross-lane primitives of the tube
 * wavefront (row_shr:1, row_shl:1, row_ror:6, row_ror:10, wave_shr:1, wave_shl:1); out[6][64] host ints. */
int gvtm_debug_dpp_selftest(gvtm_plan* plan, int* out)
{
	if (!plan || !out || plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_INVALID_ARGUMENT, "needs a device plan");
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	DeviceBuffer d;
	if ((e = d.ensure(gvtm::kDppSelftestInts * sizeof(int))) != hipSuccess) return fail_hip(e, "hipMalloc");
	e = gvtm::launch_dpp_selftest(static_cast<int*>(d.ptr), nullptr);
	if (e == hipSuccess) e = hipMemcpy(out, d.ptr, gvtm::kDppSelftestInts * sizeof(int), hipMemcpyDeviceToHost);
	if (e != hipSuccess) return fail_hip(e, "dpp selftest");
	return GVTM_OK;
}

/* Test hook: the short elementary functions of csrc/vtm_math.hpp evaluated on the host
 * (kind 0 = 2^x, 1 = 10^x, 2 = cos, 3 = tan; 4 = powf(2, x), 5 = powf(10, x), 6 = cosf, 7 = tanf of the
 * all-float path, 8 = sinf of the float model 5's sine waveform, 9 = tanf in the form with its library fallback in line,
 * arguments and results carried as doubles). */
int gvtm_debug_short_math(int kind, const double* x, size_t n, double* out)
{
	if (!x || !out) return GVTM_ERR_INVALID_ARGUMENT;
	for (size_t i = 0; i < n; ++i) {
		switch (kind) {
		case 0: out[i] = gvtm::vmath::exp2_short(x[i]); break;
		case 1: out[i] = gvtm::vmath::exp10_short(x[i]); break;
		case 2: out[i] = gvtm::vmath::cos_short(x[i]); break;
		case 3: out[i] = gvtm::vmath::tan_short(x[i]); break;
		case 4: out[i] = gvtm::vmath::powf_base2(static_cast<float>(x[i])); break;
		case 5: out[i] = gvtm::vmath::powf_base10(static_cast<float>(x[i])); break;
		case 6: out[i] = gvtm::vmath::cosf_glibc(static_cast<float>(x[i])); break;
		case 7: out[i] = gvtm::vmath::tanf_glibc(static_cast<float>(x[i])); break;
		case 8: out[i] = gvtm::vmath::sinf_glibc(static_cast<float>(x[i])); break;
		case 9: out[i] = gvtm::vmath::tanf_glibc<true>(static_cast<float>(x[i])); break;
		default: return GVTM_ERR_INVALID_ARGUMENT;
		}
	}
	return GVTM_OK;
}

/* Test hook: Util::frequency / Util::amplitude60dB / tan / cos of the all-float path (kind 0..3), its scaling-free
 * division (4), the float model 5's sin (5) and tan / cos with their library fallbacks in line (6, 7) evaluated by a kernel on the plan's device, host arrays in and out. */
int gvtm_debug_device_float_math(gvtm_plan* plan, int kind, const float* x, size_t n, float* out)
{
	if (!plan || !x || !out || kind < 0 || kind > 7) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	DeviceBuffer dx, dout;
	if ((e = dx.ensure(n * sizeof(float))) != hipSuccess) return fail_hip(e, "hipMalloc");
	if ((e = dout.ensure(n * sizeof(float))) != hipSuccess) return fail_hip(e, "hipMalloc");
	e = hipMemcpy(dx.ptr, x, n * sizeof(float), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = gvtm::launch_float_math_probe(kind, static_cast<const float*>(dx.ptr), n, static_cast<float*>(dout.ptr), nullptr);
	if (e == hipSuccess) e = hipMemcpy(out, dout.ptr, n * sizeof(float), hipMemcpyDeviceToHost);
	if (e != hipSuccess) return fail_hip(e, "float math probe");
	return GVTM_OK;
}

/* Test hook: the grouping kernel of gvtm_synthesize_voices_device alone, for `rows` utterances per workgroup, on device
 * buffers: d_row_map [groups][rows] and d_group_voice [groups] with groups = ceil(batch / rows) + n_voices; d_out_counts /
 * d_maxabs may be null.  Synchronous. */
int gvtm_debug_group_voices(gvtm_plan* plan, const int32_t* d_voice_ids, size_t batch, int rows, int32_t* d_row_map, int32_t* d_group_voice,
		int64_t* d_out_counts, float* d_maxabs)
{
	if (!plan || !d_voice_ids || !d_row_map || !d_group_voice || batch == 0 || rows < 1) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	DeviceBuffer counts;
	if ((e = counts.ensure(sizeof(int32_t) * plan->n_voices() * gvtm::kGroupVoicesThreads)) != hipSuccess) return fail_hip(e, "hipMalloc");
	const size_t groups = (batch + rows - 1) / rows + static_cast<size_t>(plan->n_voices());
	gvtm::GroupVoicesArgs ga{d_voice_ids, batch, plan->n_voices(), rows, groups, d_row_map, d_group_voice, static_cast<int32_t*>(counts.ptr), d_out_counts, d_maxabs};
	e = gvtm::launch_group_voices(ga, nullptr);
	if (e == hipSuccess) e = hipDeviceSynchronize();
	if (e != hipSuccess) return fail_hip(e, "vtm_group_voices_kernel");
	return GVTM_OK;
}

/* Test hook: the append variant of the chunk tracks kernel alone, on device buffers of the caller's (so that a test can
 * put sentinels around them): gvtm_generate_tracks_chunks_device with d_row_start [batch] int32 -- utterance b's frames
 * leave at row d_row_start[b] of its block of max_frames rows, nothing at or beyond row max_frames, and d_frame_counts[b]
 * counts this call's frames.  Synchronous. */
int gvtm_debug_tracks_append(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_chunk_offsets, const int64_t* d_utt_chunks,
		const int32_t* d_voice_ids, const int32_t* d_row_start, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts,
		gvtm_drift_state* d_drift)
{
	if (!plan || !d_events || !d_chunk_offsets || !d_utt_chunks || !d_voice_ids || !d_row_start || !d_params || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, "the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	gvtm::TrackAppendArgs args = plan_track_args(plan, d_events, d_voice_ids, batch, max_frames, d_params, d_frame_counts, d_drift);
	args.chunk_offsets = d_chunk_offsets;
	args.utt_chunks = d_utt_chunks;
	args.row_start = d_row_start;
	e = gvtm::launch_tracks(args, nullptr);
	if (e == hipSuccess) e = hipDeviceSynchronize();
	if (e != hipSuccess) return fail_hip(e, "vtm_tracks_append_kernel");
	return GVTM_OK;
}

/* Test hook: the slice variant of the chunk tracks kernel alone, on device buffers of the caller's: a slice of `batch`
 * utterances of a larger batch.  d_chunk_offsets is the whole batch's table; d_utt_chunks [batch + 1], d_voice_ids, d_drift,
 * d_frame_counts and d_frame_offsets [batch + 1] point at the slice's first utterance; d_events at the slice's first event,
 * which is event `event_base` of the batch.  d_params [batch][max_frames][16] takes the padded rows, d_packed (may be
 * null; d_frame_offsets is then not read) the frames back to back.  Synchronous. */
int gvtm_debug_tracks_slice(gvtm_plan* plan, const gvtm_event* d_events, int64_t event_base, const int64_t* d_chunk_offsets,
		const int64_t* d_utt_chunks, const int32_t* d_voice_ids, const int64_t* d_frame_offsets, size_t batch, size_t max_frames, float* d_params,
		float* d_packed, int32_t* d_frame_counts, gvtm_drift_state* d_drift)
{
	if (!plan || !d_events || !d_chunk_offsets || !d_utt_chunks || !d_voice_ids || !d_params || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (d_packed && !d_frame_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_packed needs d_frame_offsets");
	if ((reinterpret_cast<uintptr_t>(d_params) | reinterpret_cast<uintptr_t>(d_packed)) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params and d_packed must be 16-byte aligned");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, "the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	gvtm::TrackSliceArgs args{};
	static_cast<gvtm::TrackChunksArgs&>(args) = plan_track_args(plan, d_events, d_voice_ids, batch, max_frames, d_params, d_frame_counts, d_drift);
	args.chunk_offsets = d_chunk_offsets;
	args.utt_chunks = d_utt_chunks;
	args.event_base = event_base;
	args.packed = d_packed;
	args.frame_offsets = d_frame_offsets;
	e = gvtm::launch_tracks(args, nullptr);
	if (e == hipSuccess) e = hipDeviceSynchronize();
	if (e != hipSuccess) return fail_hip(e, "vtm_tracks_slice_kernel");
	return GVTM_OK;
}

/* Test hook: the carry kernel of an events-fed stream alone, on device buffers of the caller's: in utterance b's block of
 * max_frames rows of d_params the rows [d_done[b], d_held[b]) move to the front.  Synchronous. */
int gvtm_debug_carry_rows(gvtm_plan* plan, float* d_params, const int32_t* d_done, const int32_t* d_held, size_t batch, size_t max_frames)
{
	if (!plan || !d_params || !d_done || !d_held || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	e = gvtm::launch_carry_rows(gvtm::CarryArgs{d_params, d_done, d_held, batch, max_frames}, nullptr);
	if (e == hipSuccess) e = hipDeviceSynchronize();
	if (e != hipSuccess) return fail_hip(e, "vtm_carry_rows_kernel");
	return GVTM_OK;
}

#pragma GCC visibility pop
#endif /* GVTM_DIAGNOSTICS */

size_t gvtm_tracks_frame_count(const gvtm_track_config* config, const gvtm_event* events, size_t n_events)
{
	if (!config || (!events && n_events > 0)) { fail(GVTM_ERR_INVALID_ARGUMENT, "null config or events"); return static_cast<size_t>(-1); }
	gvtm::TrackConstants k;
	const char* why = gvtm::design_tracks(*config, k);
	if (why[0]) { fail(GVTM_ERR_INVALID_ARGUMENT, why); return static_cast<size_t>(-1); }
	return gvtm::tracks_frame_count(k.control_period, events, n_events);
}

size_t gvtm_tracks_chunks_frame_count(const gvtm_track_config* config, const gvtm_event* events, const int64_t* chunk_offsets, size_t n_chunks)
{
	if (!config || (n_chunks > 0 && (!events || !chunk_offsets))) { fail(GVTM_ERR_INVALID_ARGUMENT, "null config, events or chunk_offsets"); return static_cast<size_t>(-1); }
	gvtm::TrackConstants k;
	const char* why = gvtm::design_tracks(*config, k);
	if (why[0]) { fail(GVTM_ERR_INVALID_ARGUMENT, why); return static_cast<size_t>(-1); }
	size_t n = 0;
	for (size_t c = 0; c < n_chunks; ++c) {
		if (chunk_offsets[c] < 0 || chunk_offsets[c + 1] < chunk_offsets[c]) { fail(GVTM_ERR_INVALID_ARGUMENT, "chunk_offsets must not decrease"); return static_cast<size_t>(-1); }
		n += gvtm::tracks_frame_count(k.control_period, events + chunk_offsets[c], static_cast<size_t>(chunk_offsets[c + 1] - chunk_offsets[c]));
	}
	return n;
}

int gvtm_generate_tracks_device(int device, const gvtm_track_config* config, const gvtm_event* d_events,
		const int64_t* d_event_offsets, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts,
		gvtm_drift_state* d_drift, void* hip_stream)
{
	if (!config || !d_event_offsets || (!d_params && max_frames > 0)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null argument");
	gvtm::TrackArgs args{};
	const char* why = gvtm::design_tracks(*config, args.k);
	if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, why);
	if (batch == 0) return GVTM_OK;
	if (!d_events) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events");
	// frames leave the kernel as float4 stores
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (const int rc = check_device_index(device, "track generation"); rc != GVTM_OK) return rc;
	DeviceScope scope(device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	args.events = d_events;
	args.event_offsets = d_event_offsets;
	args.batch = batch;
	args.max_frames = max_frames;
	args.params = d_params;
	args.frame_counts = d_frame_counts;
	args.drift = d_drift;
	e = gvtm::launch_tracks(args, static_cast<hipStream_t>(hip_stream));
	if (e != hipSuccess) return fail_hip(e, "track generation launch");
	return GVTM_OK;
}

int gvtm_generate_tracks_host(int device, const gvtm_track_config* config, const gvtm_event* events,
		const int64_t* event_offsets, size_t batch, size_t max_frames, float* params, int32_t* frame_counts,
		gvtm_drift_state* drift)
{
	if (!config || !event_offsets || (!params && max_frames > 0)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null argument");
	if (batch == 0) return GVTM_OK;
	if (!events) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events");
	for (size_t b = 0; b < batch; ++b) {
		if (event_offsets[b + 1] < event_offsets[b] || event_offsets[0] != 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "event_offsets must start at 0 and not decrease");
	}
	if (const int rc = check_device_index(device, "track generation"); rc != GVTM_OK) return rc;
	DeviceScope scope(device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	const size_t n_events = static_cast<size_t>(event_offsets[batch]);
	DeviceBuffer d_ev, d_off, d_par, d_cnt, d_dr;
	if ((e = d_ev.ensure(sizeof(gvtm_event) * (n_events ? n_events : 1))) != hipSuccess) return fail_hip(e, "hipMalloc");
	if ((e = d_off.ensure(sizeof(int64_t) * (batch + 1))) != hipSuccess) return fail_hip(e, "hipMalloc");
	if ((e = d_par.ensure(sizeof(float) * 16 * (batch * max_frames ? batch * max_frames : 1))) != hipSuccess) return fail_hip(e, "hipMalloc");
	if ((e = d_cnt.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc");
	if (drift && (e = d_dr.ensure(sizeof(gvtm_drift_state) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc");
	if (n_events && (e = hipMemcpy(d_ev.ptr, events, sizeof(gvtm_event) * n_events, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D events");
	if ((e = hipMemcpy(d_off.ptr, event_offsets, sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D offsets");
	if (drift && (e = hipMemcpy(d_dr.ptr, drift, sizeof(gvtm_drift_state) * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D drift");
	if ((e = hipMemset(d_par.ptr, 0, sizeof(float) * 16 * batch * max_frames)) != hipSuccess) return fail_hip(e, "hipMemset");
	const int rc = gvtm_generate_tracks_device(device, config, static_cast<const gvtm_event*>(d_ev.ptr), static_cast<const int64_t*>(d_off.ptr), batch,
			max_frames, static_cast<float*>(d_par.ptr), static_cast<int32_t*>(d_cnt.ptr), drift ? static_cast<gvtm_drift_state*>(d_dr.ptr) : nullptr, nullptr);
	if (rc != GVTM_OK) return rc;
	if ((e = hipDeviceSynchronize()) != hipSuccess) return fail_hip(e, "track generation kernel");
	if (params && (e = hipMemcpy(params, d_par.ptr, sizeof(float) * 16 * batch * max_frames, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H frames");
	if (frame_counts && (e = hipMemcpy(frame_counts, d_cnt.ptr, sizeof(int32_t) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H counts");
	if (drift && (e = hipMemcpy(drift, d_dr.ptr, sizeof(gvtm_drift_state) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H drift");
	return GVTM_OK;
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

} // extern "C"

namespace {

// what a launch on behalf of a stream adds to the one-shot launch
struct StreamLaunch {
	unsigned char* d_state;
	size_t stride;
	int mode;     // gvtm::StreamMode
	int xr;       // the stream's ring length (one for all shapes; several voices: the longest of the plan's voices)
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
};

// The float model's noise samples for launches of up to `steps` internal steps per utterance: the plan's table, grown
// (synchronously) when it is shorter; beyond the cap args.noise_lp stays null and the kernel generates them.
// (The double paths generate the samples in the kernel: measured faster there.)
int use_noise_table(gvtm_plan* plan, size_t steps, gvtm::SynthArgs& args)
{
	hipError_t e = hipSuccess;
	constexpr size_t kNoiseTableMaxSteps = size_t(1) << 26; // 256 MB of table (~55 min of audio per utterance): beyond it the kernel generates the samples
	if (steps > kNoiseTableMaxSteps) {
		// (args.noise_lp stays null)
	} else if (steps > plan->noise_len) {
		// geometric growth (at least twice the old table, in units of 2^18 steps): a caller whose lengths creep up
		// retires at most eight tables on the way to the cap
		size_t want = ((steps + (size_t(1) << 18) - 1) >> 18) << 18;
		want = std::min(std::max(want, 2 * plan->noise_len), kNoiseTableMaxSteps);
		std::vector<unsigned char> host(want * sizeof(float));
		gvtm::design_noise_table(want, true, host.data());
		DeviceBuffer fresh;
		if ((e = fresh.ensure(host.size())) != hipSuccess) return fail_hip(e, "hipMalloc (noise table)");
		if ((e = hipMemcpy(fresh.ptr, host.data(), host.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "hipMemcpy (noise table)");
		if (plan->d_noise.ptr) plan->noise_retired.push_back(std::move(plan->d_noise));
		plan->d_noise = std::move(fresh);
		plan->noise_len = want;
	}
	if (steps <= kNoiseTableMaxSteps) {
		args.noise_lp = plan->d_noise.ptr;
		args.noise_len = plan->noise_len;
	}
	return GVTM_OK;
}

// The kernel arguments that follow from the plan and the request alone (launch_synthesis adds the ring length, the noise
// table and the row map)
gvtm::SynthArgs synth_args(const gvtm_plan* plan, const LaunchRequest& r)
{
	const gvtm::Design& dg = plan->designs[0];
	gvtm::SynthArgs args;
	args.k = dg.k;
	args.kconst = static_cast<const gvtm::DeviceConstants*>(plan->d_consts.ptr);
	args.params = r.params;
	args.frame_counts = r.frame_counts;
	args.audio = r.audio;
	args.out_counts = r.out_counts;
	args.maxabs = r.maxabs;
	args.wavetable = plan->d_wavetable.ptr;
	args.fir = plan->d_fir.ptr;
	std::memset(&args.fir_k, 0, sizeof(args.fir_k));
	if (!dg.model5) {
		if (dg.f32) {
			for (size_t i = 0; i < dg.fir_f.size() && i < static_cast<size_t>(gvtm::kFirKConsts); ++i) args.fir_k.f[i] = dg.fir_f[i];
			// the float kernel's plan constants as floats (several voices: the kernel reads each voice's own from kconst)
			float* kf = args.fir_k.f + gvtm::kFirKConsts;
			for (int q = 0; q < 8; ++q) kf[gvtm::kKfRadiusCoef + q] = static_cast<float>(dg.k.radius_coef[q]);
			kf[gvtm::kKfAperture2] = static_cast<float>(dg.k.aperture_radius2);
			kf[gvtm::kKfNasalR2Sq] = static_cast<float>(dg.k.nasal_r2_sq);
			kf[gvtm::kKfBasicIncrement] = static_cast<float>(dg.k.basic_increment);
			kf[gvtm::kKfBpT] = static_cast<float>(dg.k.bp_T);
			kf[gvtm::kKfBreathiness] = static_cast<float>(dg.k.breathiness);
			kf[gvtm::kKfCrossmix] = static_cast<float>(dg.k.crossmix_factor);
			kf[gvtm::kKfThroatB0] = static_cast<float>(dg.k.throat_b0);
			kf[gvtm::kKfThroatA1] = static_cast<float>(dg.k.throat_a1);
			kf[gvtm::kKfThroatGain] = static_cast<float>(dg.k.throat_gain);
			kf[gvtm::kKfMouthARad] = static_cast<float>(dg.k.mouth_a_rad);
			kf[gvtm::kKfNoseARad] = static_cast<float>(dg.k.nose_a_rad);
			kf[gvtm::kKfNasalK5] = static_cast<float>(dg.k.nasal_k[5]);
		} else {
			for (size_t i = 0; i < dg.fir.size() && i < 49; ++i) args.fir_k.d[i] = dg.fir[i];
		}
	}
	args.src_h = plan->d_src_h.ptr;
	args.src_dh = plan->d_src_dh.ptr;
	args.max_frames = r.max_frames;
	args.audio_stride = r.audio_stride;
	args.batch = r.batch;
	if (r.sl) {
		args.stream = r.sl->d_state;
		args.stream_stride = r.sl->stride;
		args.stream_mode = r.sl->mode;
		// several voices: each voice's ring is its single-voice stream's, fixed by the one-row shape's chunk (voices share the
		// precision, SectionDelay and tube layout the chunk follows)
		if (r.voices && !dg.model5) args.stream_chunk = gvtm::synth_chunk_length(dg.k, plan->precision, 1);
	}
	// (not for several voices: the hooks' buffers are sized for voice 0's steps and ceil(batch / rows) workgroups)
	args.debug_taps = r.voices ? nullptr : plan->debug_taps;
	args.phase_cycles = r.voices ? nullptr : plan->phase_cycles;
	args.k5const = static_cast<const gvtm::Model5Constants*>(plan->d_consts5.ptr);
	return args;
}

// launch() between the two events of a pair when the plan times its kernels (gvtm_plan_set_timing)
template <typename Launch>
int timed_launch(gvtm_plan* plan, hipStream_t stream, const char* what, Launch launch)
{
	hipError_t e;
	EventPair ev;
	if (plan->timing) {
		if (!plan->pool.empty()) {
			ev = std::move(plan->pool.back());
			plan->pool.pop_back();
		} else {
			if ((e = hipEventCreate(&ev.start.h)) != hipSuccess) return fail_hip(e, "hipEventCreate");
			if ((e = hipEventCreate(&ev.stop.h)) != hipSuccess) return fail_hip(e, "hipEventCreate");
		}
		if ((e = hipEventRecord(ev.start.h, stream)) != hipSuccess) return fail_hip(e, "hipEventRecord");
	}
	e = launch();
	if (plan->timing) {
		(void) hipEventRecord(ev.stop.h, stream);
		plan->pending.push_back(std::move(ev));
	}
	if (e != hipSuccess) return fail_hip(e, what);
	return GVTM_OK;
}

// a one-shot launch's rows hold max_frames frames of every voice
int check_audio_stride(const gvtm_plan* plan, size_t audio_stride, size_t max_frames, bool voices)
{
	for (int v = 0; v < plan->n_voices(); ++v) {
		if (audio_stride < design_output_count(plan->designs[v], max_frames)) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, voices ? "audio_stride smaller than gvtm_voice_output_count(plan, voice, max_frames) of voice " + std::to_string(v)
			                                              : "audio_stride smaller than gvtm_output_count(plan, max_frames)");
		}
	}
	return GVTM_OK;
}

// Every synthesis launch, enqueue-only.  With voices, the grouping kernel first builds the row map from the voice ids, then
// the voice variant of the synthesis kernel runs ceil(batch / rows) + n_voices workgroups (the bound for any mix of ids;
// those past the last voice's groups exit at once), each on one voice's constants, wavetable and ring.
int launch_synthesis(gvtm_plan* plan, const LaunchRequest& r)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	// (the single-voice entries would not know which voice to synthesize; the voices entries take a one-voice plan too)
	if (!r.voices && plan->n_voices() > 1) return refuse_voices(plan, r.sl ? "gvtm_stream_*" : "gvtm_synthesize_batch_device");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (r.batch == 0) return GVTM_OK;
	if (!r.audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if (r.voices && !r.voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null voice ids");
	if (r.max_frames > 0 && !r.params) return fail(GVTM_ERR_INVALID_ARGUMENT, "null params with max_frames > 0");
	// (several voices: the row map's int32 slots also count up to n_voices partly empty workgroups)
	if (r.batch > (r.voices ? 0x3fffffffu : 0x7fffffffu)) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	if (!fits_step_counter(plan, r.max_frames)) return fail(GVTM_ERR_INVALID_ARGUMENT, "max_frames * control_steps does not fit the 31-bit step counter");
	// (a stream checks its stride against what each call produces: stream_launch)
	if (!r.sl) {
		const int rc = check_audio_stride(plan, r.audio_stride, r.max_frames, r.voices);
		if (rc != GVTM_OK) return rc;
	}
	const bool model5 = plan->designs[0].model5;
	if (r.voices && model5 && plan->designs[0].f32 && !plan->float5_voices) {
		return fail(GVTM_ERR_UNSUPPORTED, "a gvtm_plan_create_model5_float plan has no launch of several voices (one voice per plan; "
				"gvtm_plan_create_model5_float_voices makes the float plans that have)");
	}
	// (a stream's launches are the voice variant's exactly when its plan has several voices: create_stream)
	const gvtm::LaunchShape shape = r.sl ? plan->stream_launch_shape(r.batch, r.rows, r.sl->xr) : plan->launch_shape(r.batch, r.rows, r.voices);
	if (!shape.rows) return fail(GVTM_ERR_UNSUPPORTED, "LDS budget exceeded");
	const int rows = shape.rows;

	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	hipStream_t stream = static_cast<hipStream_t>(r.hip_stream);

	gvtm::SynthArgs args = synth_args(plan, r);
	args.xr = shape.ring;
	size_t work = r.batch; // what launch_synth takes: utterances, or with voices workgroups
	if (r.voices) {
		work = (r.batch + rows - 1) / rows + static_cast<size_t>(plan->n_voices());
		const size_t map_ints = work * rows, count_ints = static_cast<size_t>(plan->n_voices()) * gvtm::kGroupVoicesThreads;
		if ((e = r.groups->ensure(sizeof(int32_t) * (map_ints + work + count_ints))) != hipSuccess) return fail_hip(e, "hipMalloc row map");
		int32_t* const d_map = static_cast<int32_t*>(r.groups->ptr);
		gvtm::GroupVoicesArgs ga{r.voice_ids, r.batch, plan->n_voices(), rows, work, d_map, d_map + map_ints, d_map + map_ints + work, r.out_counts, r.maxabs};
		if ((e = gvtm::launch_group_voices(ga, stream)) != hipSuccess) return fail_hip(e, "vtm_group_voices_kernel launch");
		args.row_map = d_map;
		args.group_voice = d_map + map_ints;
	}
	if (!model5 && !r.sl && GVTM_NOISE_TABLE && plan->precision == GVTM_PRECISION_F32) {
		// one-shot launches read the noise samples from the plan's table, one for every voice (every utterance starts from
		// the same seed), as long as the voice with the most steps needs (streams generate them: their length has no bound)
		const int rc = use_noise_table(plan, r.max_frames * static_cast<size_t>(max_control_steps(plan)), args);
		if (rc != GVTM_OK) return rc;
	}
	return timed_launch(plan, stream, r.voices ? "vtm_synth_kernel launch (voices)" : "vtm_synth_kernel launch", [&] {
		return model5 ? gvtm::launch_synth5(args, work, plan->precision, shape.forced - 1, stream) : gvtm::launch_synth(args, work, plan->precision, rows, stream);
	});
}

// What lies between the two launches of an events entry: the plan's frame buffer (the enqueue-only entries' scratch) and
// the frame counts, the caller's or the plan's
int events_scratch(gvtm_plan* plan, size_t batch, size_t max_frames, int32_t* d_frame_counts, float*& d_params, int32_t*& d_counts)
{
	hipError_t e;
	if ((e = plan->async.params.ensure(sizeof(float) * batch * std::max<size_t>(max_frames, 1) * GVTM_N_PARAM)) != hipSuccess) return fail_hip(e, "hipMalloc frames");
	if ((e = plan->async.frames.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frame counts");
	d_params = static_cast<float*>(plan->async.params.ptr);
	d_counts = d_frame_counts ? d_frame_counts : static_cast<int32_t*>(plan->async.frames.ptr);
	return GVTM_OK;
}

} // namespace

extern "C" {

int gvtm_synthesize_batch_device(gvtm_plan* plan, const float* d_params, const int32_t* d_frame_counts,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int64_t* d_out_counts, float* d_maxabs, void* hip_stream)
{
	return launch_synthesis(plan, LaunchRequest{d_params, d_frame_counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream});
}

int gvtm_synthesize_voices_device(gvtm_plan* plan, const float* d_params, const int32_t* d_frame_counts, const int32_t* d_voice_ids,
		size_t max_frames, size_t batch, float* d_audio, size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, void* hip_stream)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	return launch_synthesis(plan, LaunchRequest{d_params, d_frame_counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream,
			0, true, d_voice_ids, &plan->async.groups});
}

int gvtm_synthesize_events_device(gvtm_plan* plan, const gvtm_track_config* config, const gvtm_event* d_events,
		const int64_t* d_event_offsets, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream)
{
	if (!plan || !config) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or config");
	if (plan->n_voices() > 1) return refuse_voices(plan, "gvtm_synthesize_events_device");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (batch == 0) return GVTM_OK;
	if (!d_events || !d_event_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events or event_offsets");
	gvtm::TrackConstants tk{};
	const char* why = gvtm::design_tracks(*config, tk);
	if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, why);
	if (!control_period_matches(plan, tk)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "control_period_ms of the track configuration and the plan's control rate disagree");
	}
	// Two launches on the caller's stream with a frame buffer of the plan's in between.  (Walking the event lists inside the
	// synthesis kernel's interpolation wavefront was built and measured: bit-identical, no frame buffer, and 17.2 -> 33.1 ms
	// per 4096 x 80 events -- an event boundary is a round trip to memory in the middle of a tick, three times over because
	// the parameter groups run at different lags -- and 125 ms with the next events prefetched into registers, which that
	// wavefront does not have to spare.  DESIGN.md 6b.)
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	float* frames;
	int32_t* counts;
	int rc = events_scratch(plan, batch, max_frames, d_frame_counts, frames, counts);
	if (rc == GVTM_OK) rc = gvtm_generate_tracks_device(plan->device, config, d_events, d_event_offsets, batch, max_frames, frames, counts, d_drift, hip_stream);
	if (rc != GVTM_OK) return rc;
	return launch_synthesis(plan, LaunchRequest{frames, counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream});
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
			hipError_t e = scope.status();
			if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
			// (the same size every time: the buffer is allocated once, and a call in flight must not see it rewritten)
			if ((e = upload(plan->d_voice_tracks, table)) != hipSuccess) return fail_hip(e, "upload voice track constants");
		}
		plan->voice_tracks = std::move(table);
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // extern "C"

namespace {

// The event lists of a batch that mixes voices: one list per utterance (d_offsets [batch + 1], the events-voices entries) or
// several (chunked: d_offsets the chunks' event offsets, d_utt_chunks [batch + 1] the utterances' chunks)
struct VoiceEvents {
	const gvtm_event* d_events;
	const int64_t* d_offsets;
	const int32_t* d_voice_ids;
	bool chunked = false;
	const int64_t* d_utt_chunks = nullptr;
};

// What the events-voices and events-chunks entries share up to the tracks launch: the checks in the order the header gives
// them, then the voice or the chunk variant of the tracks kernel on the caller's stream.
int launch_voice_tracks(gvtm_plan* plan, const VoiceEvents& lists, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts, gvtm_drift_state* d_drift, void* hip_stream)
{
	if (batch == 0) return GVTM_OK;
	if (!lists.d_events || !lists.d_offsets || !lists.d_voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events, offsets or voice ids");
	if (lists.chunked && !lists.d_utt_chunks) return fail(GVTM_ERR_INVALID_ARGUMENT, "null utt_chunks");
	if (!d_params && max_frames > 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null params with max_frames > 0");
	// frames leave the kernel as float4 stores
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (batch > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	gvtm::TrackChunksArgs args = plan_track_args(plan, lists.d_events, lists.d_voice_ids, batch, max_frames, d_params, d_frame_counts, d_drift);
	(lists.chunked ? args.chunk_offsets : args.event_offsets) = lists.d_offsets;
	args.utt_chunks = lists.d_utt_chunks; // (null unless chunked)
	const hipError_t e = lists.chunked ? gvtm::launch_tracks<gvtm::TrackChunksArgs>(args, static_cast<hipStream_t>(hip_stream))
	                                   : gvtm::launch_tracks<gvtm::TrackVoicesArgs>(args, static_cast<hipStream_t>(hip_stream));
	if (e != hipSuccess) return fail_hip(e, lists.chunked ? "track generation launch (chunks)" : "track generation launch (voices)");
	return GVTM_OK;
}

// null plan, no table yet, design-only plan: in this order (a design-only plan still tells whether its table is set)
int check_voice_tracks_plan(const gvtm_plan* plan, const char* entry)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, std::string(entry) + ": the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	return GVTM_OK;
}

int generate_voice_tracks(gvtm_plan* plan, const char* entry, const VoiceEvents& lists, size_t batch, size_t max_frames, float* d_params,
		int32_t* d_frame_counts, gvtm_drift_state* d_drift, void* hip_stream)
{
	const int rc = check_voice_tracks_plan(plan, entry);
	if (rc != GVTM_OK) return rc;
	DeviceScope scope(plan->device);
	const hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	return launch_voice_tracks(plan, lists, batch, max_frames, d_params, d_frame_counts, d_drift, hip_stream);
}

int synthesize_voice_events(gvtm_plan* plan, const char* entry, const VoiceEvents& lists, size_t batch, size_t max_frames, float* d_audio,
		size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream)
{
	int rc = check_voice_tracks_plan(plan, entry);
	if (rc != GVTM_OK) return rc;
	if (batch == 0) return GVTM_OK;
	// (what the synthesis launch would refuse is refused before the tracks kernel advances the drift states)
	if (!d_audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if ((rc = check_audio_stride(plan, audio_stride, max_frames, true)) != GVTM_OK) return rc;
	// As gvtm_synthesize_events_device: two launches on the caller's stream with the plan's frame buffer in between; the
	// frame counts of the tracks kernel (0 for a bad voice id, which the grouping kernel fails on its own) are the
	// synthesis launch's.
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	float* frames;
	int32_t* counts;
	if ((rc = events_scratch(plan, batch, max_frames, d_frame_counts, frames, counts)) != GVTM_OK) return rc;
	if ((rc = launch_voice_tracks(plan, lists, batch, max_frames, frames, counts, d_drift, hip_stream)) != GVTM_OK) return rc;
	return launch_synthesis(plan, LaunchRequest{frames, counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream, 0, true,
			lists.d_voice_ids, &plan->async.groups});
}

} // namespace

extern "C" {

int gvtm_generate_tracks_voices_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_event_offsets, const int32_t* d_voice_ids,
		size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts, gvtm_drift_state* d_drift, void* hip_stream)
{
	return generate_voice_tracks(plan, "gvtm_generate_tracks_voices_device", VoiceEvents{d_events, d_event_offsets, d_voice_ids}, batch, max_frames,
			d_params, d_frame_counts, d_drift, hip_stream);
}

int gvtm_synthesize_events_voices_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_event_offsets, const int32_t* d_voice_ids,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs,
		gvtm_drift_state* d_drift, void* hip_stream)
{
	return synthesize_voice_events(plan, "gvtm_synthesize_events_voices_device", VoiceEvents{d_events, d_event_offsets, d_voice_ids}, batch, max_frames,
			d_audio, audio_stride, d_frame_counts, d_out_counts, d_maxabs, d_drift, hip_stream);
}

int gvtm_generate_tracks_chunks_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_chunk_offsets, const int64_t* d_utt_chunks,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts, gvtm_drift_state* d_drift,
		void* hip_stream)
{
	return generate_voice_tracks(plan, "gvtm_generate_tracks_chunks_device", VoiceEvents{d_events, d_chunk_offsets, d_voice_ids, true, d_utt_chunks}, batch,
			max_frames, d_params, d_frame_counts, d_drift, hip_stream);
}

int gvtm_synthesize_events_chunks_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_chunk_offsets, const int64_t* d_utt_chunks,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts,
		int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream)
{
	return synthesize_voice_events(plan, "gvtm_synthesize_events_chunks_device", VoiceEvents{d_events, d_chunk_offsets, d_voice_ids, true, d_utt_chunks},
			batch, max_frames, d_audio, audio_stride, d_frame_counts, d_out_counts, d_maxabs, d_drift, hip_stream);
}

} // extern "C"

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
	hipError_t e;
	if (out_counts && (e = hipMemcpy(out_counts, plan->host.counts.ptr, sizeof(int64_t) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H counts");
	if (maxabs && (e = hipMemcpy(maxabs, plan->host.maxabs.ptr, sizeof(float) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H maxabs");
	if (scales && (e = hipMemcpy(scales, plan->host.scales.ptr, sizeof(float) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H scales");
	return GVTM_OK;
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
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	const size_t row_in = max_frames * GVTM_N_PARAM;
	const size_t pbytes = sizeof(float) * batch * row_in;
	auto& sc = plan->host;
	if ((e = sc.params.ensure(pbytes ? pbytes : 16)) != hipSuccess) return fail_hip(e, "hipMalloc params");
	if ((e = sc.audio.ensure(std::max<size_t>(16, sizeof(float) * batch * audio_stride))) != hipSuccess) return fail_hip(e, "hipMalloc audio");
	if ((e = sc.counts.ensure(sizeof(int64_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc counts");
	if ((e = sc.maxabs.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc maxabs");
	if (counts_in && (e = sc.frames.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frames");
	if (voices && (e = sc.voice_ids.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc voice ids");
	if (j.pcm && (e = sc.pcm.ensure(std::max<size_t>(16, sizeof(int16_t) * batch * audio_stride))) != hipSuccess) return fail_hip(e, "hipMalloc pcm");
	if (j.pcm && (e = sc.scales.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc scales");
	if (voices && (e = reserve_host_groups(plan, slice)) != hipSuccess) return fail_hip(e, "hipMalloc row map");

	if (counts_in && (e = hipMemcpy(sc.frames.ptr, counts_in, sizeof(int32_t) * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D frame_counts");
	if (voices && (e = hipMemcpy(sc.voice_ids.ptr, j.voice_ids, sizeof(int32_t) * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D voice_ids");
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
	if (!bad.empty()) g_last_error = voices ? "frame_counts entry outside [0, max_frames] or voice id outside [0, n_voices): those utterances have out_counts = -1"
	                                        : "frame_counts entry outside [0, max_frames]: those utterances have out_counts = -1";
	return GVTM_OK;
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

/* ---------------------------------------------------------------------------------------------
 * Streams: the stateful form of the path (include/gama_vtm.h, "Streams").
 */

} // extern "C"

enum StreamFeed : int { kFeedNone = 0, kFeedFrames = 1, kFeedEvents = 2 };

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
	// how the stream has been fed since the last reset: frames (gvtm_stream_push) or event lists (gvtm_stream_push_events);
	// one way per run
	int feed = kFeedNone;
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
	hipError_t e = hipMemcpy(s->d_state.ptr, init.data(), init.size(), hipMemcpyHostToDevice);
	if (e != hipSuccess) return fail_hip(e, "H2D stream state");
	return GVTM_OK;
}

// the stream's drift generators from host states, or (null) fresh ones (DriftGenerator.cpp:28, :40)
int stream_upload_drift(gvtm_stream* s, const gvtm_drift_state* states)
{
	hipError_t e = s->d_drift.ensure(sizeof(gvtm_drift_state) * s->batch);
	if (e != hipSuccess) return fail_hip(e, "hipMalloc drift states");
	std::vector<gvtm_drift_state> fresh;
	if (!states) {
		fresh.assign(s->batch, gvtm_drift_state{0.7892347, 0.0, 0.0, 0.0, 0.0});
		states = fresh.data();
	}
	if ((e = hipMemcpy(s->d_drift.ptr, states, sizeof(gvtm_drift_state) * s->batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D drift states");
	return GVTM_OK;
}

uint64_t outputs_before(const gvtm::DeviceConstants& k, uint64_t steps)
{
	return ((steps << 16) + k.time_inc - 1) / k.time_inc;
}

// The samples of one launch on behalf of the stream, known before it: utterance b synthesizes n_frames[b] more frames.
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
		const uint64_t after = s->steps_done[b] + static_cast<uint64_t>(n_frames[b]) * k.control_steps;
		if (after + 4096ull >= (1ull << 31)) r.too_long = true;
		const uint64_t k1 = final ? gvtm::src_output_count(k.time_inc, k.pad, k.upsampling, after) : outputs_before(k, after);
		r.want[b] = static_cast<int64_t>(k1 - outputs_before(k, s->steps_done[b]));
		r.need = std::max(r.need, static_cast<size_t>(r.want[b]));
	}
	return r;
}

// One launch on behalf of the stream: utterance b synthesizes n_frames[b] frames from the front of held[b] -- or, in an
// events-fed run, from the front of its block of d_held, which the launch reads in place (no staging, no copy of frames);
// behind a push's launch the carry kernel then moves the rows it left to the front of the block.
int stream_launch(gvtm_stream* s, const std::vector<size_t>& n_frames, bool final, float* audio, size_t audio_stride, int64_t* out_counts,
		float* maxabs, bool* launched = nullptr)
{
	gvtm_plan* plan = s->plan;
	const size_t batch = s->batch;
	size_t rows_max = 0;
	bool lockstep = true, any = final;
	// (lockstep is judged per voice: a workgroup only ever holds one voice; first[v] is voice v's first utterance)
	std::vector<size_t> first(static_cast<size_t>(plan->n_voices()), batch);
	for (size_t b = 0; b < batch; ++b) {
		const size_t rows = n_frames[b] + (final ? 0 : 1); // a push carries the look-ahead frame behind its last one
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
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	try {
		s->staging.assign(on_device ? 0 : batch * rows_max * GVTM_N_PARAM, 0.0f);
		s->counts.assign(batch, 0);
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
	for (size_t b = 0; b < batch; ++b) {
		if (!n_frames[b]) continue;
		const size_t rows = n_frames[b] + (final ? 0 : 1);
		if (!on_device) std::memcpy(s->staging.data() + b * rows_max * GVTM_N_PARAM, s->held[b].data(), sizeof(float) * rows * GVTM_N_PARAM);
		s->counts[b] = static_cast<int32_t>(n_frames[b]);
	}
	const size_t pbytes = sizeof(float) * s->staging.size();
	const size_t abytes = sizeof(float) * batch * std::max<size_t>(audio_stride, 1);
	if (!on_device && (e = s->d_params.ensure(pbytes)) != hipSuccess) return fail_hip(e, "hipMalloc params");
	if ((e = s->d_frames.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frames");
	if ((e = s->d_audio.ensure(abytes)) != hipSuccess) return fail_hip(e, "hipMalloc audio");
	if ((e = s->d_counts.ensure(sizeof(int64_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc counts");
	if ((e = s->d_maxabs.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc maxabs");
	if (!on_device && (e = hipMemcpy(s->d_params.ptr, s->staging.data(), pbytes, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D params");
	if ((e = hipMemcpy(s->d_frames.ptr, s->counts.data(), sizeof(int32_t) * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D frame counts");
	if ((e = hipMemsetAsync(s->d_audio.ptr, 0, abytes, nullptr)) != hipSuccess) return fail_hip(e, "hipMemsetAsync");
	const StreamLaunch sl{static_cast<unsigned char*>(s->d_state.ptr), s->state_stride, final ? gvtm::kStreamFinish : gvtm::kStreamPush, s->xr};
	// (one utterance per workgroup unless the utterances are in lockstep)
	float* const d_rows_in = static_cast<float*>(on_device ? s->d_held.ptr : s->d_params.ptr);
	const int rc = launch_synthesis(plan, LaunchRequest{d_rows_in, static_cast<const int32_t*>(s->d_frames.ptr), batch,
			rows_max, static_cast<float*>(s->d_audio.ptr), audio_stride, static_cast<int64_t*>(s->d_counts.ptr), static_cast<float*>(s->d_maxabs.ptr), nullptr,
			lockstep ? 0 : 1, s->voices, s->voices ? static_cast<const int32_t*>(s->d_voice_ids.ptr) : nullptr, &s->d_groups, &sl});
	if (rc != GVTM_OK) return rc;
	if (launched) *launched = true;
	if (on_device && !final) {
		// (d_rows: the rows each block held when the launch began, behind the row starts of the push)
		const gvtm::CarryArgs ca{d_rows_in, static_cast<const int32_t*>(s->d_frames.ptr), static_cast<const int32_t*>(s->d_rows.ptr) + batch, batch, rows_max};
		if ((e = gvtm::launch_carry_rows(ca, nullptr)) != hipSuccess) return fail_hip(e, "vtm_carry_rows_kernel launch");
	}
	if ((e = hipDeviceSynchronize()) != hipSuccess) return fail_hip(e, "vtm_synth_kernel execution");
	std::vector<int64_t> got(batch, 0);
	if ((e = hipMemcpy(got.data(), s->d_counts.ptr, sizeof(int64_t) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H counts");
	for (size_t b = 0; b < batch; ++b) {
		if (got[b] != samples.want[b]) return fail(GVTM_ERR_HIP, "internal error: the device's sample count differs from the host's");
	}
	if (audio && audio_stride && (e = hipMemcpy(audio, s->d_audio.ptr, sizeof(float) * batch * audio_stride, hipMemcpyDeviceToHost)) != hipSuccess) {
		return fail_hip(e, "D2H audio");
	}
	if (out_counts) std::copy(got.begin(), got.end(), out_counts);
	if (maxabs && (e = hipMemcpy(maxabs, s->d_maxabs.ptr, sizeof(float) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H maxabs");
	for (size_t b = 0; b < batch; ++b) {
		s->steps_done[b] += static_cast<uint64_t>(n_frames[b]) * plan->designs[voice_of(s, b)].k.control_steps;
		if (on_device) s->held_rows[b] -= n_frames[b];
		else s->held[b].erase(s->held[b].begin(), s->held[b].begin() + static_cast<std::ptrdiff_t>(n_frames[b] * GVTM_N_PARAM));
	}
	return GVTM_OK;
}

// Host voice ids of gvtm_stream_create_voices / gvtm_stream_reset_voices: all of them in [0, n_voices), or the call is refused
int check_voice_ids(const gvtm_plan* plan, const int32_t* voice_ids, size_t batch)
{
	for (size_t b = 0; b < batch; ++b) {
		if (voice_ids[b] < 0 || voice_ids[b] >= plan->n_voices()) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, "utterance " + std::to_string(b) + ": voice id " + std::to_string(voice_ids[b]) + " outside [0, " +
					std::to_string(plan->n_voices()) + ")");
		}
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
			} else {
				// each voice's ring is the one-row shape's, whatever shape a launch takes (the kernel derives it per voice)
				const int xr = plan->stream_ring(v);
				s->state_stride = std::max(s->state_stride, gvtm::stream_state_bytes(k, plan->precision, xr));
				// the serial wavefronts work in blocks of 2, 4 and 4 or 6 steps (vtm_kernel_v2.inc): their states are exact at
				// multiples of 12 steps, so a push synthesizes a multiple of 12 / gcd(control_steps, 12) frames and keeps the rest
				s->granule_frames.push_back(12u / gcd_u(k.control_steps, 12u));
			}
		}
		s->held.resize(batch);
		s->held_rows.assign(batch, 0);
		s->steps_done.assign(batch, 0);
		DeviceScope scope(plan->device);
		hipError_t e = scope.status();
		if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
		if ((e = s->d_state.ensure(s->state_stride * batch)) != hipSuccess) return fail_hip(e, "hipMalloc stream state");
		// (one voice: every utterance's id is 0, which only the tracks kernel of an events-fed run reads)
		if ((e = s->d_voice_ids.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc voice ids");
		if (s->voices) e = hipMemcpy(s->d_voice_ids.ptr, voice_ids, sizeof(int32_t) * batch, hipMemcpyHostToDevice);
		else e = hipMemset(s->d_voice_ids.ptr, 0, sizeof(int32_t) * batch);
		if (e != hipSuccess) return fail_hip(e, "H2D voice ids");
		int rc = stream_upload_fresh_state(s.get());
		if (rc != GVTM_OK) return rc;
		if ((rc = stream_upload_drift(s.get(), nullptr)) != GVTM_OK) return rc;
		*stream_out = s.release();
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
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
	const int rc = check_voice_ids(plan, voice_ids, batch);
	if (rc != GVTM_OK) return rc;
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
	if (scope.status() != hipSuccess) return fail_hip(scope.status(), "hipSetDevice");
	for (auto& h : s->held) h.clear();
	std::fill(s->held_rows.begin(), s->held_rows.end(), size_t(0));
	std::fill(s->steps_done.begin(), s->steps_done.end(), uint64_t(0));
	s->finished = false;
	s->feed = kFeedNone; // (the drift generators run on: the reference's Controller never reseeds its own)
	return stream_upload_fresh_state(s);
}

int gvtm_stream_reset_voices(gvtm_stream* s, const int32_t* voice_ids)
{
	if (!s || !voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream or voice_ids");
	const int rc = check_voice_ids(s->plan, voice_ids, s->batch);
	if (rc != GVTM_OK) return rc;
	// past the checks the stream takes the new ids; a device error from here on leaves it finished (pushes refused) until a
	// reset succeeds, so that no push runs on half-reset state
	if (s->voices) {
		std::copy(voice_ids, voice_ids + s->batch, s->voice_ids.begin());
		DeviceScope scope(s->plan->device);
		// (the buffer holds batch ids since create: no reallocation)
		const hipError_t e = scope.status() != hipSuccess ? scope.status()
		                                                   : hipMemcpy(s->d_voice_ids.ptr, voice_ids, sizeof(int32_t) * s->batch, hipMemcpyHostToDevice);
		if (e != hipSuccess) { s->finished = true; return fail_hip(e, "H2D voice ids"); }
	}
	const int rc_reset = gvtm_stream_reset(s);
	if (rc_reset != GVTM_OK) s->finished = true;
	return rc_reset;
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
		// the last frame stands for its own successor (Controller.cpp:283)
		for (size_t b = 0; b < s->batch; ++b) n[b] = s->feed == kFeedEvents ? s->held_rows[b] : s->held[b].size() / GVTM_N_PARAM;
		const int rc = stream_launch(s, n, true, audio, audio_stride, out_counts, maxabs);
		if (rc == GVTM_OK) s->finished = true;
		return rc;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // extern "C"

namespace {

// the most rows a block of d_held may have: launch_synthesis takes the row stride as max_frames, whose steps must fit its
// 31-bit step counter
size_t stream_block_limit(const gvtm_plan* plan)
{
	unsigned max_steps = 1;
	for (int v = 0; v < plan->n_voices(); ++v) max_steps = std::max(max_steps, plan->designs[v].k.control_steps);
	return static_cast<size_t>(((1ull << 31) - 4096ull - 1ull) / max_steps);
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
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
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
	if ((e = s->d_events.ensure(sizeof(gvtm_event) * std::max<size_t>(n_events, 1))) != hipSuccess) return fail_hip(e, "hipMalloc events");
	if ((e = s->d_chunk_offsets.ensure(sizeof(int64_t) * (n_chunks + 1))) != hipSuccess) return fail_hip(e, "hipMalloc chunk offsets");
	if ((e = s->d_utt_chunks.ensure(sizeof(int64_t) * (batch + 1))) != hipSuccess) return fail_hip(e, "hipMalloc utterance chunks");
	if ((e = s->d_rows.ensure(sizeof(int32_t) * 2 * batch)) != hipSuccess) return fail_hip(e, "hipMalloc row starts");
	if ((e = s->d_new_counts.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frame counts");
	if (n_events && (e = hipMemcpy(s->d_events.ptr, events, sizeof(gvtm_event) * n_events, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D events");
	if ((e = hipMemcpy(s->d_chunk_offsets.ptr, chunk_offsets, sizeof(int64_t) * (n_chunks + 1), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D chunk offsets");
	if ((e = hipMemcpy(s->d_utt_chunks.ptr, utt_chunks, sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D utterance chunks");
	if ((e = hipMemcpy(s->d_rows.ptr, rows.data(), sizeof(int32_t) * 2 * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D row starts");
	// append, synthesis, carry: all on the stream's launch stream
	gvtm::TrackAppendArgs ta = plan_track_args(plan, static_cast<const gvtm_event*>(s->d_events.ptr), static_cast<const int32_t*>(s->d_voice_ids.ptr), batch,
			s->held_cap, static_cast<float*>(s->d_held.ptr), static_cast<int32_t*>(s->d_new_counts.ptr), static_cast<gvtm_drift_state*>(s->d_drift.ptr));
	ta.chunk_offsets = static_cast<const int64_t*>(s->d_chunk_offsets.ptr);
	ta.utt_chunks = static_cast<const int64_t*>(s->d_utt_chunks.ptr);
	ta.row_start = static_cast<const int32_t*>(s->d_rows.ptr);
	if ((e = gvtm::launch_tracks(ta, nullptr)) != hipSuccess) return fail_hip(e, "track generation launch (append)");
	*advanced = true;
	s->feed = kFeedEvents;
	s->held_rows = have;
	const int rc = stream_launch(s, n, false, audio, audio_stride, out_counts, nullptr);
	if (rc != GVTM_OK) return rc;
	// (a push that synthesizes nothing launches nothing behind the tracks kernel: the copy waits for it)
	std::vector<int32_t> counted(batch, 0);
	if ((e = hipMemcpy(counted.data(), s->d_new_counts.ptr, sizeof(int32_t) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H frame counts");
	for (size_t b = 0; b < batch; ++b) {
		if (static_cast<size_t>(counted[b]) != fresh[b]) return fail(GVTM_ERR_HIP, "internal error: the device's frame count differs from the host's");
	}
	return GVTM_OK;
}

} // namespace

extern "C" {

int gvtm_stream_push_events(gvtm_stream* s, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks, float* audio,
		size_t audio_stride, int64_t* out_counts, int32_t* frame_counts_out)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->finished) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream has been finished: gvtm_stream_reset() starts the next utterances");
	if (s->feed == kFeedFrames) return fail(GVTM_ERR_INVALID_ARGUMENT, "the stream is fed frames (gvtm_stream_push) until the next gvtm_stream_reset()");
	const gvtm_plan* plan = s->plan;
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, "gvtm_stream_push_events: the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	const size_t batch = s->batch;
	// (a null utt_chunks: no utterance receives a chunk)
	const int64_t last_chunk = utt_chunks ? utt_chunks[batch] : 0;
	if (last_chunk > 0 && (!events || !chunk_offsets)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events or chunk_offsets");
	if (utt_chunks) {
		if (utt_chunks[0] < 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "utt_chunks must not be negative");
		for (size_t b = 0; b < batch; ++b) {
			if (utt_chunks[b + 1] < utt_chunks[b]) return fail(GVTM_ERR_INVALID_ARGUMENT, "utt_chunks must not decrease");
		}
	}
	const size_t n_chunks = last_chunk > 0 ? static_cast<size_t>(last_chunk) : 0;
	for (size_t c = 0; c < n_chunks; ++c) {
		if (chunk_offsets[c] < 0 || chunk_offsets[c + 1] < chunk_offsets[c]) return fail(GVTM_ERR_INVALID_ARGUMENT, "chunk_offsets must not decrease");
	}
	const size_t n_events = n_chunks ? static_cast<size_t>(chunk_offsets[n_chunks]) : 0;
	try {
		// what the tracks kernel will generate, counted here: every sample count is known before anything is launched
		const int cp = plan->voice_tracks[0].control_period; // (every voice's is the plan's: gvtm_plan_set_voice_tracks)
		std::vector<size_t> fresh(batch, 0), have(batch, 0), n(batch, 0);
		for (size_t b = 0; b < batch; ++b) {
			for (int64_t c = utt_chunks ? utt_chunks[b] : 0; c < (utt_chunks ? utt_chunks[b + 1] : 0); ++c) {
				fresh[b] += gvtm::tracks_frame_count(cp, events + chunk_offsets[c], static_cast<size_t>(chunk_offsets[c + 1] - chunk_offsets[c]));
			}
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
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	if ((e = hipMemcpy(states_out, s->d_drift.ptr, sizeof(gvtm_drift_state) * s->batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H drift states");
	return GVTM_OK;
}

int gvtm_stream_set_drift(gvtm_stream* s, const gvtm_drift_state* states)
{
	if (!s) return fail(GVTM_ERR_INVALID_ARGUMENT, "null stream");
	if (s->feed == kFeedEvents) return fail(GVTM_ERR_INVALID_ARGUMENT, "the drift generators are running: gvtm_stream_reset() comes first");
	try {
		DeviceScope scope(s->plan->device);
		if (scope.status() != hipSuccess) return fail_hip(scope.status(), "hipSetDevice");
		return stream_upload_drift(s, states);
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

int gvtm_normalize_batch_device(gvtm_plan* plan, const float* d_audio, size_t batch, size_t audio_stride,
		const int64_t* d_counts, const float* d_maxabs, float* d_out_f32, int16_t* d_out_i16,
		float* d_scales, void* hip_stream)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan (GVTM_DEVICE_NONE)");
	if (batch == 0 || audio_stride == 0) return GVTM_OK;
	if (!d_audio || !d_maxabs) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio or maxabs");
	if ((d_out_f32 == nullptr) == (d_out_i16 == nullptr)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "exactly one of d_out_f32 / d_out_i16 must be given");
	}
	if (batch > 65535) return fail(GVTM_ERR_INVALID_ARGUMENT, "normalize: batch above 65535 per call");
	DeviceScope scope(plan->device);
	hipError_t e = scope.status();
	if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
	gvtm::NormalizeArgs args;
	args.audio = d_audio;
	args.counts = d_counts;
	args.maxabs = d_maxabs;
	args.out_f32 = d_out_f32;
	args.out_i16 = d_out_i16;
	args.scales = d_scales;
	args.audio_stride = audio_stride;
	e = gvtm::launch_normalize(args, batch, static_cast<hipStream_t>(hip_stream));
	if (e != hipSuccess) return fail_hip(e, "vtm_normalize_kernel launch");
	return GVTM_OK;
}

} // extern "C"

/* ---------------------------------------------------------------------------------------------
 * Ragged batches, packed in and packed out (include/gama_vtm.h, "Ragged batches").
 */

namespace {

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
	if (frame_offsets[0] != 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "frame_offsets must start at 0 and not decrease");
	for (size_t b = 0; b < batch; ++b) {
		if (frame_offsets[b + 1] < frame_offsets[b]) return fail(GVTM_ERR_INVALID_ARGUMENT, "frame_offsets must start at 0 and not decrease");
	}
	if (voice_ids) {
		const int rc = check_voice_ids(plan, voice_ids, batch);
		if (rc != GVTM_OK) return rc;
	} else if (plan->n_voices() > 1) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null voice ids: the plan has " + std::to_string(plan->n_voices()) + " voices (one voice id per utterance)");
	}
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

struct PackedJob {
	const float* frames;
	const int64_t* frame_offsets;
	const int32_t* voice_ids; // null: the plan's one voice through the single-voice launch, else the voices launch
	size_t batch;
	float* audio;     // float32 output, or null
	int16_t* pcm;     // int16 output, or null
	bool to_pcm;      // which of the two is due
	size_t capacity;
	int64_t* sample_offsets_out;
	int64_t* out_counts;
	float* maxabs;
	float* scales;    // pcm only
};

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
// offset tables and the voice ids uploaded), the grouping's scratch and, for the longest utterance, the noise table
int stage_packed_batch(gvtm_plan* plan, const std::vector<PackedSlice>& slices, size_t longest, size_t batch, const int64_t* frame_offsets,
		const std::vector<int64_t>& offsets, const int32_t* voice_ids, bool pcm)
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
	if ((e = sc.frame_offsets.ensure(sizeof(int64_t) * (batch + 1))) != hipSuccess) return fail_hip(e, "hipMalloc frame offsets");
	if ((e = sc.sample_offsets.ensure(sizeof(int64_t) * (batch + 1))) != hipSuccess) return fail_hip(e, "hipMalloc sample offsets");
	if ((e = sc.frames.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frame counts");
	if ((e = sc.counts.ensure(sizeof(int64_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc counts");
	if ((e = sc.maxabs.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc maxabs");
	if (pcm && (e = sc.scales.ensure(sizeof(float) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc scales");
	if (voices && (e = sc.voice_ids.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc voice ids");
	if (voices && (e = reserve_host_groups(plan, largest)) != hipSuccess) return fail_hip(e, "hipMalloc row map");
	// the noise table once, for the longest utterance: no slice regrows it in the middle of the pipeline
	if (const int rc = gvtm_plan_reserve(plan, longest); rc != GVTM_OK) return rc;
	if ((e = hipMemcpy(sc.frame_offsets.ptr, frame_offsets, sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D frame offsets");
	if ((e = hipMemcpy(sc.sample_offsets.ptr, offsets.data(), sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D sample offsets");
	if (voices && (e = hipMemcpy(sc.voice_ids.ptr, voice_ids, sizeof(int32_t) * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D voice_ids");
	sc.slices = slices.size(), sc.largest_slice = largest;
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
	const int rc = launch_synthesis(plan, LaunchRequest{s.rows(set), sc.frames.as<int32_t>() + s.lo, n, s.max_frames, s.audio(set), s.stride, d_counts, d_maxabs, stream,
			forced_rows, voices, voices ? sc.voice_ids.as<int32_t>() + s.lo : nullptr, &sc.groups});
	if (rc != GVTM_OK) return rc;
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
		const bool voices = j.voice_ids != nullptr;
		if (batch != 0) {
			if (j.to_pcm ? !j.pcm : !j.audio) return fail(GVTM_ERR_INVALID_ARGUMENT, j.to_pcm ? "null pcm buffer" : "null audio buffer");
			if (j.frame_offsets[batch] > 0 && !j.frames) return fail(GVTM_ERR_INVALID_ARGUMENT, "null frames");
			if (j.capacity < static_cast<size_t>(offsets[batch])) {
				return fail(GVTM_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(j.capacity) + " below gvtm_packed_sample_offsets (" + std::to_string(offsets[batch]) + " samples)");
			}
		}
		if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
		if (batch == 0) {
			if (j.sample_offsets_out) j.sample_offsets_out[0] = 0;
			return GVTM_OK;
		}
		if (batch > 0x3fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large");

		// every slice in the shape of the whole batch, as host_pipeline's
		size_t machine, longest;
		const gvtm::LaunchShape shape_all = whole_batch_shape(plan, batch, machine);
		auto& sc = plan->host;
		const size_t width = j.pcm ? sizeof(int16_t) : sizeof(float);
		std::vector<PackedSlice> slices;
		auto slice_of = [&](size_t lo, size_t hi, size_t max_frames) {
			PackedSlice s = packed_slice(plan, width, offsets, lo, hi, max_frames);
			s.in_bytes = sizeof(float) * GVTM_N_PARAM * static_cast<size_t>(j.frame_offsets[hi] - j.frame_offsets[lo]);
			return s;
		};
		if ((rc = cut_slices(plan, j.frame_offsets, batch, machine, slice_of, slices, longest)) != GVTM_OK) return rc;

		DeviceScope scope(plan->device);
		const hipError_t e = scope.status();
		if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
		if ((rc = stage_packed_batch(plan, slices, longest, batch, j.frame_offsets, offsets, j.voice_ids, j.pcm != nullptr)) != GVTM_OK) return rc;
		if (j.sample_offsets_out) std::copy(offsets.begin(), offsets.end(), j.sample_offsets_out);

		auto set_of = [&](size_t i) { return static_cast<unsigned char*>(sc.set[i % 3].ptr); };
		auto input = [&](size_t i, hipStream_t stream) {
			const PackedSlice& s = slices[i];
			return s.in_bytes ? hipMemcpyAsync(set_of(i), j.frames + GVTM_N_PARAM * static_cast<size_t>(j.frame_offsets[s.lo]), s.in_bytes, hipMemcpyHostToDevice, stream) : hipSuccess;
		};
		auto work = [&](size_t i, hipStream_t stream) -> int {
			const PackedSlice& s = slices[i];
			const hipError_t we = gvtm::launch_unpack_frames(gvtm::UnpackFramesArgs{reinterpret_cast<float*>(set_of(i)), sc.frame_offsets.as<int64_t>() + s.lo, s.rows(set_of(i)),
					sc.frames.as<int32_t>() + s.lo, s.hi - s.lo, s.max_frames}, stream);
			if (we != hipSuccess) return fail_hip(we, "vtm_unpack_frames_kernel launch");
			return synthesize_and_pack(plan, s, set_of(i), j.pcm != nullptr, voices, shape_all.forced, stream);
		};
		auto output = [&](size_t i, hipStream_t stream) {
			return copy_out_packed(slices[i], set_of(i), j.pcm ? static_cast<void*>(j.pcm) : static_cast<void*>(j.audio), width, offsets, stream);
		};
		if ((rc = run_slices(plan, slices.size(), 1, 3, "H2D frames", input, work, output)) != GVTM_OK) return rc;
		return copy_back_results(plan, batch, j.out_counts, j.maxabs, j.scales);
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
	float* audio;
	int16_t* pcm;
	bool to_pcm;
	size_t capacity;
	int64_t* sample_offsets_out;
	int64_t* frame_offsets_out;
	float* frames_out;            // packed frames [frame_offsets[batch]][16], or null
	size_t frames_capacity;       // in frames
	int64_t* out_counts;
	float* maxabs;
	float* scales;                // pcm only
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
	if (utt_chunks[0] != 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "utt_chunks must start at 0 and not decrease");
	for (size_t b = 0; b < batch; ++b) {
		if (utt_chunks[b + 1] < utt_chunks[b]) return fail(GVTM_ERR_INVALID_ARGUMENT, "utt_chunks must start at 0 and not decrease");
	}
	const size_t n_chunks = static_cast<size_t>(utt_chunks[batch]);
	if (chunk_offsets[0] != 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "chunk_offsets must start at 0 and not decrease");
	for (size_t c = 0; c < n_chunks; ++c) {
		if (chunk_offsets[c + 1] < chunk_offsets[c]) return fail(GVTM_ERR_INVALID_ARGUMENT, "chunk_offsets must start at 0 and not decrease");
	}
	const int cp = plan->voice_tracks[0].control_period; // (every voice's is the plan's: gvtm_plan_set_voice_tracks)
	for (size_t b = 0; b < batch; ++b) {
		size_t frames = 0;
		for (int64_t c = utt_chunks[b]; c < utt_chunks[b + 1]; ++c) {
			frames += gvtm::tracks_frame_count(cp, events + chunk_offsets[c], static_cast<size_t>(chunk_offsets[c + 1] - chunk_offsets[c]));
		}
		frame_offsets[b + 1] = frame_offsets[b] + static_cast<int64_t>(frames);
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
		const bool voices = j.voice_ids != nullptr, pcm = j.to_pcm;
		if (batch != 0) {
			if (pcm ? !j.pcm : !j.audio) return fail(GVTM_ERR_INVALID_ARGUMENT, pcm ? "null pcm buffer" : "null audio buffer");
			if (j.capacity < static_cast<size_t>(offsets[batch])) {
				return fail(GVTM_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(j.capacity) + " below gvtm_events_packed_layout (" + std::to_string(offsets[batch]) + " samples)");
			}
			if (j.frames_out && j.frames_capacity < static_cast<size_t>(frame_offsets[batch])) {
				return fail(GVTM_ERR_INVALID_ARGUMENT, "frames_capacity " + std::to_string(j.frames_capacity) + " below the layout's " + std::to_string(frame_offsets[batch]) + " frames");
			}
		}
		if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
		if (batch == 0) {
			if (j.sample_offsets_out) j.sample_offsets_out[0] = 0;
			if (j.frame_offsets_out) j.frame_offsets_out[0] = 0;
			return GVTM_OK;
		}
		if (batch > 0x3fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large");

		size_t machine, longest;
		const gvtm::LaunchShape shape_all = whole_batch_shape(plan, batch, machine);
		auto& sc = plan->host;
		const size_t width = pcm ? sizeof(int16_t) : sizeof(float);
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
		hipError_t e = scope.status();
		if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
		if ((rc = stage_packed_batch(plan, slices, longest, batch, frame_offsets.data(), offsets, j.voice_ids, pcm)) != GVTM_OK) return rc;
		if ((e = sc.chunk_offsets.ensure(sizeof(int64_t) * (n_chunks + 1))) != hipSuccess) return fail_hip(e, "hipMalloc chunk offsets");
		if ((e = sc.utt_chunks.ensure(sizeof(int64_t) * (batch + 1))) != hipSuccess) return fail_hip(e, "hipMalloc utterance chunks");
		if ((e = hipMemcpy(sc.chunk_offsets.ptr, j.chunk_offsets, sizeof(int64_t) * (n_chunks + 1), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D chunk offsets");
		if ((e = hipMemcpy(sc.utt_chunks.ptr, j.utt_chunks, sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D utterance chunks");
		if (!voices) { // the tracks kernel still reads an id per utterance: the one voice's
			if ((e = sc.voice_ids.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc voice ids");
			const std::vector<int32_t> zeros(batch, 0);
			if ((e = hipMemcpy(sc.voice_ids.ptr, zeros.data(), sizeof(int32_t) * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D voice_ids");
		}
		if (j.drift) {
			if ((e = sc.drift.ensure(sizeof(gvtm_drift_state) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc drift states");
			if ((e = hipMemcpy(sc.drift.ptr, j.drift, sizeof(gvtm_drift_state) * batch, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "H2D drift states");
		}
		if (j.sample_offsets_out) std::copy(offsets.begin(), offsets.end(), j.sample_offsets_out);
		if (j.frame_offsets_out) std::copy(frame_offsets.begin(), frame_offsets.end(), j.frame_offsets_out);

		auto set_of = [&](size_t i) { return static_cast<unsigned char*>(sc.set[i % 3].ptr); };
		// slice i's events go up and its frames are generated behind them on the H2D stream: the walk is a chain of dependent
		// steps (as long as the slice's longest list, however few the utterances) that one wavefront per two utterances runs, so it
		// runs beside the synthesis kernels of the slice before instead of in front of its own
		auto input = [&](size_t i, hipStream_t stream) {
			const PackedSlice& s = slices[i];
			const size_t first = event_of(s.lo), n_events = event_of(s.hi) - first;
			const hipError_t ie = n_events ? hipMemcpyAsync(set_of(i), j.events + first, sizeof(gvtm_event) * n_events, hipMemcpyHostToDevice, stream) : hipSuccess;
			if (ie != hipSuccess) return ie;
			gvtm::TrackSliceArgs ta{};
			static_cast<gvtm::TrackChunksArgs&>(ta) = plan_track_args(plan, reinterpret_cast<const gvtm_event*>(set_of(i)), sc.voice_ids.as<int32_t>() + s.lo, s.hi - s.lo,
					s.max_frames, s.rows(set_of(i)), sc.frames.as<int32_t>() + s.lo, j.drift ? sc.drift.as<gvtm_drift_state>() + s.lo : nullptr);
			ta.chunk_offsets = sc.chunk_offsets.as<int64_t>();
			ta.utt_chunks = sc.utt_chunks.as<int64_t>() + s.lo;
			ta.event_base = static_cast<int64_t>(first);
			ta.packed = j.frames_out ? s.frames(set_of(i)) : nullptr;
			ta.frame_offsets = sc.frame_offsets.as<int64_t>() + s.lo;
			return gvtm::launch_tracks(ta, stream);
		};
		auto work = [&](size_t i, hipStream_t stream) -> int {
			return synthesize_and_pack(plan, slices[i], set_of(i), pcm, voices, shape_all.forced, stream);
		};
		auto output = [&](size_t i, hipStream_t stream) {
			const PackedSlice& s = slices[i];
			const hipError_t oe = copy_out_packed(s, set_of(i), pcm ? static_cast<void*>(j.pcm) : static_cast<void*>(j.audio), width, offsets, stream);
			if (oe != hipSuccess || !s.frames_bytes) return oe;
			return hipMemcpyAsync(j.frames_out + GVTM_N_PARAM * static_cast<size_t>(frame_offsets[s.lo]), s.frames(set_of(i)), s.frames_bytes, hipMemcpyDeviceToHost, stream);
		};
		if ((rc = run_slices(plan, slices.size(), 1, 3, "H2D events / track generation launch", input, work, output)) != GVTM_OK) return rc;
		if ((rc = copy_back_results(plan, batch, j.out_counts, j.maxabs, j.scales)) != GVTM_OK) return rc;
		if (j.drift && (e = hipMemcpy(j.drift, sc.drift.ptr, sizeof(gvtm_drift_state) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H drift states");
		// what the tracks kernel counted against what the layout was built on
		std::vector<int32_t> counted(batch, 0);
		if ((e = hipMemcpy(counted.data(), sc.frames.ptr, sizeof(int32_t) * batch, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e, "D2H frame counts");
		for (size_t b = 0; b < batch; ++b) {
			if (static_cast<int64_t>(counted[b]) != frame_offsets[b + 1] - frame_offsets[b]) return fail(GVTM_ERR_HIP, "internal error: the device's frame count differs from the host's");
		}
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // namespace

extern "C" {

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
	return packed_pipeline(plan, PackedJob{frames, frame_offsets, voice_ids, batch, audio, nullptr, false, audio_capacity, sample_offsets_out, out_counts, maxabs, nullptr});
}

int gvtm_synthesize_packed_host_pcm16(gvtm_plan* plan, const float* frames, const int64_t* frame_offsets, const int32_t* voice_ids, size_t batch,
		int16_t* pcm, size_t pcm_capacity, int64_t* sample_offsets_out, int64_t* out_counts, float* maxabs, float* scales)
{
	return packed_pipeline(plan, PackedJob{frames, frame_offsets, voice_ids, batch, nullptr, pcm, true, pcm_capacity, sample_offsets_out, out_counts, maxabs, scales});
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
	return events_packed_pipeline(plan, EventsPackedJob{events, chunk_offsets, utt_chunks, voice_ids, batch, audio, nullptr, false, audio_capacity, sample_offsets_out,
			frame_offsets_out, frames_out, frames_capacity, out_counts, maxabs, nullptr, drift});
}

int gvtm_synthesize_events_packed_host_pcm16(gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets, const int64_t* utt_chunks,
		const int32_t* voice_ids, size_t batch, int16_t* pcm, size_t pcm_capacity, int64_t* sample_offsets_out, int64_t* frame_offsets_out,
		float* frames_out, size_t frames_capacity, int64_t* out_counts, float* maxabs, float* scales, gvtm_drift_state* drift)
{
	return events_packed_pipeline(plan, EventsPackedJob{events, chunk_offsets, utt_chunks, voice_ids, batch, nullptr, pcm, true, pcm_capacity, sample_offsets_out,
			frame_offsets_out, frames_out, frames_capacity, out_counts, maxabs, scales, drift});
}

int gvtm_plan_set_staging_limit(gvtm_plan* plan, size_t bytes)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->host.limit = bytes;
	// what an earlier call holds beyond the new limit goes now (every packed call drains its streams before it returns)
	if (bytes && plan->device != GVTM_DEVICE_NONE && plan->host.staging_bytes() > bytes) {
		DeviceScope scope(plan->device);
		if (scope.status() != hipSuccess) return fail_hip(scope.status(), "hipSetDevice");
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

int gvtm_plan_reserve(gvtm_plan* plan, size_t max_frames)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	// (the plans whose one-shot launches read the table: launch_synthesis)
	if (plan->designs[0].model5 || !GVTM_NOISE_TABLE || plan->precision != GVTM_PRECISION_F32) return GVTM_OK;
	if (!fits_step_counter(plan, max_frames)) return fail(GVTM_ERR_INVALID_ARGUMENT, "max_frames * control_steps does not fit the 31-bit step counter");
	try {
		DeviceScope scope(plan->device);
		if (scope.status() != hipSuccess) return fail_hip(scope.status(), "hipSetDevice");
		gvtm::SynthArgs unused;
		return use_noise_table(plan, max_frames * static_cast<size_t>(max_control_steps(plan)), unused);
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // extern "C"
