// C ABI of libgama_vtm.so, spectrum analysis: the object (window, bin count, tables and scratch on the device), the rule on
// the host with a double transform, and the rule for a batch on the device, slice by slice over the reserved scratch.
#include <cmath>
#include <cstring>
#include <memory>
#include <new>

#include "vtm_host.hpp"
#include "vtm_analysis.hpp"

using namespace gvtm::host;

struct gvtm_analysis {
	gvtm_analysis_config config{};
	int device = GVTM_DEVICE_NONE;
	size_t n_bins = 0;
	std::vector<double> window;        // [W]
	std::vector<double> host_twiddle;  // (cos, -sin)(2 pi k / 65536), k in [0, 32768): the host transform's
	// on the device: the window, the float twiddle table, and the scratch of `reserved` buffers in flight
	DeviceBuffer d_window, d_table, d_coefs, d_T, d_Z;
	size_t reserved = 0;
};

namespace {

constexpr size_t kMaxReserved = 65536; // (a launch's grid is 129 workgroups per buffer at the most)

// the scratch of n buffers in flight (the object's device is current); the caller has drained the device where it shrinks
int reserve_scratch(gvtm_analysis* an, size_t n)
{
	an->reserved = 0;
	an->d_coefs = DeviceBuffer();
	an->d_T = DeviceBuffer();
	an->d_Z = DeviceBuffer();
	const size_t image = sizeof(gvtm::AnalysisComplex) * gvtm::kAnalysisHalf;
	hipError_t e = an->d_coefs.ensure(sizeof(float) * n);
	if (e == hipSuccess) e = an->d_T.ensure(image * n);
	if (e == hipSuccess) e = an->d_Z.ensure(image * n);
	if (e != hipSuccess) return e == hipErrorOutOfMemory ? fail(GVTM_ERR_OUT_OF_MEMORY, "analysis scratch: out of device memory") : fail_hip(e, "hipMalloc analysis scratch");
	an->reserved = n;
	return GVTM_OK;
}

// A plain double transform of 65 536 complex points in place: bit reversal, then radix-2 steps with twiddles from the table
void host_transform(std::vector<double>& re, std::vector<double>& im, const std::vector<double>& twiddle)
{
	constexpr unsigned N = gvtm::kAnalysisSize;
	for (unsigned i = 0, j = 0; i < N; ++i) {
		if (i < j) {
			std::swap(re[i], re[j]);
			std::swap(im[i], im[j]);
		}
		unsigned bit = N >> 1;
		for (; j & bit; bit >>= 1) j ^= bit;
		j ^= bit;
	}
	for (unsigned len = 2; len <= N; len <<= 1) {
		const unsigned half = len / 2, step = N / len;
		for (unsigned base = 0; base < N; base += len) {
			for (unsigned k = 0; k < half; ++k) {
				const double wr = twiddle[2 * (k * step)], wi = twiddle[2 * (k * step) + 1];
				const unsigned a = base + k, b = a + half;
				const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
				re[b] = re[a] - tr;
				im[b] = im[a] - ti;
				re[a] += tr;
				im[a] += ti;
			}
		}
	}
}

} // namespace

extern "C" {

int gvtm_analysis_create(int device, const gvtm_analysis_config* config, gvtm_analysis** analysis_out)
{
	if (!config || !analysis_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null config or analysis_out");
	*analysis_out = nullptr;
	if (config->window_type < GVTM_WINDOW_RECTANGULAR || config->window_type > GVTM_WINDOW_BLACKMAN) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "window_type must be one of GVTM_WINDOW_*");
	}
	const int64_t W = config->window_size;
	if (W < 32 || W > gvtm::kAnalysisSize || (W & (W - 1)) != 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "window_size must be a power of two in [32, 65536]");
	if (config->sample_rate == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "sample_rate must not be 0");
	if (std::isnan(config->min_db) || std::isnan(config->max_freq_hz)) return fail(GVTM_ERR_INVALID_ARGUMENT, "min_db and max_freq_hz must be numbers");
	try {
		std::unique_ptr<gvtm_analysis> an(new gvtm_analysis);
		an->config = *config;
		an->device = device;
		gvtm::design_analysis_window(config->window_type, static_cast<unsigned>(W), an->window);
		an->n_bins = gvtm::design_analysis_bin_count(config->sample_rate, config->max_freq_hz);
		an->host_twiddle.resize(2 * static_cast<size_t>(gvtm::kAnalysisHalf));
		for (int k = 0; k < gvtm::kAnalysisHalf; ++k) {
			const double angle = 2.0 * M_PI * k / gvtm::kAnalysisSize;
			an->host_twiddle[2 * k] = std::cos(angle);
			an->host_twiddle[2 * k + 1] = -std::sin(angle);
		}
		if (device != GVTM_DEVICE_NONE) {
			int rc = check_device_index(device, "gvtm_analysis_create on a device");
			if (rc != GVTM_OK) return rc;
			hipDeviceProp_t prop;
			if (const hipError_t e = hipGetDeviceProperties(&prop, device); e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
			if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
				return fail(GVTM_ERR_NO_DEVICE, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
			}
			DeviceScope scope(device);
			if ((rc = scope.entered()) != GVTM_OK) return rc;
			std::vector<float> table;
			gvtm::design_analysis_twiddles(table);
			if ((rc = upload(an->d_window, an->window, "upload analysis window")) != GVTM_OK) return rc;
			if ((rc = upload(an->d_table, table, "upload analysis twiddles")) != GVTM_OK) return rc;
			if ((rc = reserve_scratch(an.get(), GVTM_ANALYSIS_DEFAULT_BUFFERS)) != GVTM_OK) return rc;
		}
		*analysis_out = an.release();
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

void gvtm_analysis_destroy(gvtm_analysis* analysis)
{
	if (!analysis) return;
	if (analysis->device == GVTM_DEVICE_NONE) {
		delete analysis;
		return;
	}
	DeviceScope scope(analysis->device); // (the buffers are freed on their device)
	delete analysis;
}

size_t gvtm_analysis_bin_count(const gvtm_analysis* analysis)
{
	if (!analysis) { fail(GVTM_ERR_INVALID_ARGUMENT, "null analysis"); return static_cast<size_t>(-1); }
	return analysis->n_bins;
}

int gvtm_analysis_window(const gvtm_analysis* analysis, double* window_out, size_t capacity)
{
	if (!analysis || !window_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null analysis or window_out");
	if (capacity < analysis->window.size()) return fail(GVTM_ERR_INVALID_ARGUMENT, "capacity below window_size");
	std::memcpy(window_out, analysis->window.data(), sizeof(double) * analysis->window.size());
	return GVTM_OK;
}

size_t gvtm_analysis_buffer_count(int64_t n_samples, int64_t first_sample, size_t max_buffers)
{
	return static_cast<size_t>(gvtm::analysis_buffer_count(n_samples, first_sample, static_cast<int64_t>(std::min<size_t>(max_buffers, INT64_MAX))));
}

int gvtm_analysis_reserve(gvtm_analysis* analysis, size_t n_buffers)
{
	if (!analysis) return fail(GVTM_ERR_INVALID_ARGUMENT, "null analysis");
	if (n_buffers == 0 || n_buffers > kMaxReserved) return fail(GVTM_ERR_INVALID_ARGUMENT, "n_buffers must lie in [1, 65536]");
	if (analysis->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only analysis (GVTM_DEVICE_NONE): there is no scratch to reserve");
	DeviceScope scope(analysis->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	if (n_buffers == analysis->reserved) return GVTM_OK;
	// (queued kernels may still use the scratch that goes)
	if (const hipError_t e = hipDeviceSynchronize(); e != hipSuccess) return fail_hip(e, "hipDeviceSynchronize");
	return reserve_scratch(analysis, n_buffers);
}

int gvtm_analysis_apply_host(const gvtm_analysis* analysis, const float* samples, size_t n_samples, size_t first_sample, size_t max_buffers,
		float* spectra_out, float* signal_out, size_t* n_buffers_out)
{
	if (!analysis) return fail(GVTM_ERR_INVALID_ARGUMENT, "null analysis");
	if (!samples && n_samples > 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null samples with n_samples > 0");
	if (!spectra_out && !signal_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null spectra_out and signal_out: nothing to compute");
	if (n_samples > static_cast<size_t>(INT64_MAX) || first_sample > static_cast<size_t>(INT64_MAX)) return fail(GVTM_ERR_INVALID_ARGUMENT, "n_samples or first_sample too large");
	const size_t n_buffers = gvtm_analysis_buffer_count(static_cast<int64_t>(n_samples), static_cast<int64_t>(first_sample), max_buffers);
	if (n_buffers_out) *n_buffers_out = n_buffers;
	try {
		constexpr size_t N = gvtm::kAnalysisSize;
		const size_t W = analysis->window.size();
		const float min_db = static_cast<float>(analysis->config.min_db);
		std::vector<float> s(N);
		std::vector<double> re(N), im(N);
		for (size_t k = 0; k < n_buffers; ++k) {
			const float* in = samples + first_sample + k * N;
			float max_value = 0.0f;
			for (size_t i = 0; i < N; ++i) {
				const float a = std::fabs(in[i]);
				if (a > max_value) max_value = a;
			}
			const float coef = gvtm::analysis_norm_coef(max_value);
			for (size_t i = 0; i < N; ++i) s[i] = gvtm::analysis_normalised(in[i], coef);
			if (signal_out) std::memcpy(signal_out + k * W, s.data(), sizeof(float) * W);
			if (!spectra_out) continue;
			for (size_t i = 0; i < N; ++i) {
				re[i] = i < W ? static_cast<double>(gvtm::analysis_windowed(s[i], analysis->window[i])) : 0.0;
				im[i] = 0.0;
			}
			host_transform(re, im, analysis->host_twiddle);
			float* out = spectra_out + k * analysis->n_bins;
			for (size_t i = 0; i < analysis->n_bins; ++i) {
				const float mag = static_cast<float>(std::sqrt(re[i] * re[i] + im[i] * im[i]) * 0.00390625);
				out[i] = gvtm::analysis_level(mag, analysis->config.log_scale != 0, min_db);
			}
		}
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

int gvtm_analyze_spectrum_device(gvtm_analysis* analysis, const float* d_audio, size_t audio_stride, const int64_t* d_counts, const int64_t* d_first,
		size_t batch, size_t max_buffers, float* d_spectra, float* d_signal, int32_t* d_buffers_out, void* hip_stream)
{
	if (!analysis) return fail(GVTM_ERR_INVALID_ARGUMENT, "null analysis");
	const bool work = batch > 0 && max_buffers > 0;
	if (work) {
		if (!d_audio || !d_counts) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio or counts");
		if (!d_spectra && !d_signal) return fail(GVTM_ERR_INVALID_ARGUMENT, "null d_spectra and d_signal: nothing to compute");
		if (batch > 0x7fffffffu || max_buffers > 0x7fffffffu || batch * max_buffers > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch * max_buffers too large");
		if (audio_stride > static_cast<size_t>(INT64_MAX)) return fail(GVTM_ERR_INVALID_ARGUMENT, "audio_stride too large");
	} else if (batch > 0x7fffffffu) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large");
	}
	if (analysis->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only analysis (GVTM_DEVICE_NONE): there is no CPU path behind the device entry");
	if (batch == 0) return GVTM_OK;
	if (!work && (!d_buffers_out || !d_counts)) return GVTM_OK;
	DeviceScope scope(analysis->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	return analysis_enqueue(analysis, d_audio, audio_stride, d_counts, d_first, batch, max_buffers, d_spectra, d_signal, d_buffers_out, nullptr, 0,
			static_cast<hipStream_t>(hip_stream));
}

} // extern "C"

namespace gvtm::host {

AnalysisFacts analysis_facts(const gvtm_analysis* analysis)
{
	return {analysis->device, analysis->config.sample_rate, analysis->n_bins, analysis->window.size()};
}

int analysis_enqueue(gvtm_analysis* analysis, const float* d_audio, size_t audio_stride, const int64_t* d_counts, const int64_t* d_first, size_t batch,
		size_t max_buffers, float* d_spectra, float* d_signal, int32_t* d_buffers_out, const int32_t* d_out_slots, size_t out_stride, hipStream_t stream)
{
	gvtm::AnalysisArgs args{};
	args.audio = d_audio;
	args.audio_stride = audio_stride;
	args.counts = d_counts;
	args.first = d_first;
	args.batch = batch;
	args.max_buffers = max_buffers;
	args.W = static_cast<unsigned>(analysis->window.size());
	args.n_bins = static_cast<unsigned>(analysis->n_bins);
	args.log_scale = analysis->config.log_scale != 0;
	args.min_db = static_cast<float>(analysis->config.min_db);
	args.window = analysis->d_window.as<double>();
	args.table = analysis->d_table.as<gvtm::AnalysisComplex>();
	args.norm_coefs = analysis->d_coefs.as<float>();
	args.T = analysis->d_T.as<gvtm::AnalysisComplex>();
	args.Z = analysis->d_Z.as<gvtm::AnalysisComplex>();
	args.spectra = d_spectra;
	args.signal = d_signal;
	args.buffers_out = d_buffers_out;
	args.out_slots = d_out_slots;
	args.out_stride = out_stride;
	// slices of the pairs (utterance, buffer) over the reserved scratch, one after the other on the caller's stream
	if (analysis->reserved == 0) return fail(GVTM_ERR_OUT_OF_MEMORY, "no scratch reserved (the last gvtm_analysis_reserve failed)");
	const size_t pairs = batch * max_buffers;
	size_t p0 = 0;
	do {
		args.first_pair = p0;
		args.n_pairs = std::min(analysis->reserved, pairs - p0);
		if (const hipError_t e = gvtm::launch_analysis(args, stream); e != hipSuccess) return fail_hip(e, "analysis launch");
		p0 += args.n_pairs;
	} while (p0 < pairs);
	return GVTM_OK;
}

} // namespace gvtm::host
