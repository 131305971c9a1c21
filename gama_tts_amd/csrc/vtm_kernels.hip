// CDNA4 (gfx950) kernels of the batched vocal-tract model.
//
//   vtm_synth_kernel   (vtm_kernel_v2.inc)  VocalTractModel0 / 2 / 4 semantics: a workgroup owns 1, 2, 4 or 8 utterances and
//                      5 + NH wavefronts with fixed roles (tube, scans, pre-/post-tube filters, interpolation, helpers),
//                      software-pipelined over chunks of internal-rate steps with one barrier per tick; see that file's header
//                      (its targets variant, kTargetsFlag, is compiled in vtm_kernels_targets.hip, and that variant
//                      under several voices in vtm_kernels_targets_voices.hip)
//   vtm5_synth_kernel  (vtm_kernel_m5.inc)  VocalTractModel5 semantics, same organisation (its voice variant is compiled
//                      in vtm_kernels_m5v.hip, its float class in vtm_kernels_m5f.hip, that class's voice variant in
//                      vtm_kernels_m5fv.hip, its targets variant in vtm_kernels_m5t.hip and vtm_kernels_m5ft.hip, and
//                      that variant under several voices in vtm_kernels_m5tv.hip and vtm_kernels_m5ftv.hip)
//   vtm_normalize_kernel                    output scaling of Controller::writeOutputToBuffer / writeOutputToFile
//
// Which shape a launch has (rows, chunk length, helpers, ring, LDS) is decided in vtm_kernel_shapes.hpp and only there, and
// there every variant of vtm_synth_kernel is launched (launch_v2): this unit holds the frames variants, one voice and several.
// Everything between the parameter frames (HBM in) and the audio samples (HBM out) lives in LDS; there is no
// intermediate global traffic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "vtm_design.hpp"
#include "vtm_kernels.hpp"
#include "vtm_math.hpp"

namespace gvtm {

namespace {
#include "vtm_device_common.inc"
} // namespace

#include "vtm_kernel_v2.inc"
#include "vtm_kernel_m5.inc"

// Controller::writeOutputToBuffer / writeOutputToFile (Controller.cpp:315-340): scale by
// 0.95 / max|x| (Util::calculateOutputScale, VTMUtil.cpp:48-67); the int16 form rounds as
// WAVEFileWriter::writeSample does (WAVEFileWriter.cpp:122-125).  HBM-bound elementwise pass.
__global__ __launch_bounds__(256) void vtm_normalize_kernel(const NormalizeArgs a)
{
	const size_t utt = blockIdx.y;
	const int64_t n = a.counts ? a.counts[utt] : static_cast<int64_t>(a.audio_stride);
	const float peak = a.maxabs[utt];
	const float scale = (peak < 1.0e-30f) ? 0.0f : 0.95f / peak;
	if (a.scales && blockIdx.x == 0 && threadIdx.x == 0) a.scales[utt] = scale;
	const float* __restrict__ in = a.audio + utt * a.audio_stride;
	const int64_t limit = n < static_cast<int64_t>(a.audio_stride) ? n : static_cast<int64_t>(a.audio_stride);
	for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < limit;
			i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
		const float v = in[i] * scale;
		if (a.out_f32) a.out_f32[utt * a.audio_stride + i] = v;
		if (a.out_i16) a.out_i16[utt * a.audio_stride + i] = static_cast<int16_t>(static_cast<int>(roundf(v * 32767.0f)));
	}
}

// ---- kernel shapes and their launch: vtm_kernel_shapes.hpp, shared with the targets variants' translation units ----
#include "vtm_kernel_shapes.hpp"

hipError_t launch_synth(const SynthArgs& args, size_t batch, int precision, int rows, hipStream_t stream)
{
	// (the targets variant lives in vtm_kernels_targets.hip, that of several voices in vtm_kernels_targets_voices.hip: this
	// file's code object keeps the kernels it had)
	if (args.tg_offsets) return args.row_map ? launch_synth_targets_voices(args, batch, precision, rows, stream) : launch_synth_targets(args, batch, precision, rows, stream);
	// (one pass over the shapes per variant, single voice first: the order the code object has its kernels in)
	if (!args.row_map) return launch_v2_variant<0>(args, batch, precision, rows, stream);
	return launch_v2_variant<v2::kVoicesFlag>(args, batch, precision, rows, stream);
}

int synth_chunk_length(const DeviceConstants& k, int precision, int rows)
{
	return with_shape(precision, rows, k.section_delay, k.layout, 0, [](auto s) { return decltype(s)::C; });
}

int synth_filter_split(const DeviceConstants& k, int precision, int rows)
{
	return with_shape(precision, rows, k.section_delay, k.layout, 0, [](auto s) {
		using S = decltype(s);
		return v2::filter_split_f2<typename S::CT, typename S::ST, S::D, S::U, S::LAYOUT, false>() ? 1 : 0;
	});
}

size_t stream_state_bytes(const DeviceConstants& k, int precision, int xr)
{
	const int lanes = k.layout == 1 ? 48 : 16, words = 2 * k.section_delay + 1;
	return with_shape(precision, 1, k.section_delay, k.layout, size_t(0), [&](auto s) {
		return StreamLayout<typename decltype(s)::CT, typename decltype(s)::ST>::bytes(lanes, words, xr);
	});
}

// the shape of `rows` utterances per workgroup of one voice: its rows as launched, its ring (xr, or with xr == 0 its own)
// and its LDS bytes; rows == 0 where there is no such shape
static LaunchShape shape_of_rows(const DeviceConstants& k, int precision, int rows, int xr)
{
	return with_shape(precision, rows, k.section_delay, k.layout, LaunchShape{}, [&](auto s) {
		using S = decltype(s);
		const int ring = xr > 0 ? xr : ring_length(k, S::C);
		return LaunchShape{S::U, ring, S::lds_bytes(ring), S::U, S::U};
	});
}

LaunchShape synth_launch_shape(const Design* voices, int n_voices, int precision, size_t batch, int forced_rows, bool several_voices,
		int stream_ring, bool fit, bool targets)
{
	const auto fits = [&](const LaunchShape& s) { return !fit || s.lds <= kLdsPerWorkgroup; };
	if (voices[0].model5) {
		// Model 5: the index of the shape in its class (m5_shape, vtm_kernel_m5.inc); a diagnostics build forces either:
		// forced_rows 1 the first, 2 the second.
		// The double class: index 0 (one utterance per workgroup), whatever the batch: the two-utterance shape (two tube
		// wavefronts, chunk of 24 steps -- what LDS holds of the 62-entry tube records) measured SLOWER at every batch size
		// (batch 512 x 250 frames: 17.3 ms against 2 x 6.97 ms; profiles/r03_role_cycles_m5.txt): the passes are
		// latency-bound, so a chunk of 24 steps costs what one of 60 does, and the tube wavefronts slow down from 268 to
		// 430 cycles per step next to five busy helpers.  Only forcing picks it (tests hold it to the one-utterance shape's
		// samples bit for bit), and not for the voice variant, which has the one-utterance shape only.
		// The float class (one utterance per workgroup; one voice or, in its voice variant, several: the same rule): up to
		// one workgroup per compute unit the chunk of 60 steps; beyond, the chunk of 56, whose 80 800 B let two workgroups
		// share a compute unit (DESIGN.md 4b has the measurement).
		const bool float_class = precision == GVTM_PRECISION_F32;
		const int index = float_class ? (forced_rows == 1 ? 0 : (forced_rows == 2 || batch > 256 ? 1 : 0)) : (forced_rows == 2 && !several_voices ? 1 : 0);
		// The targets variant has shapes of its own by the same index and the same rule: each is the shape above
		// with the f0 record, its chunk shortened where the record does not fit the budget the shape stands for
		// (m5_targets_shape, vtm_kernel_m5.inc).  (Offsets is a constant expression: no kernel is named here.)  Under several
		// voices the index is the voices launch's above, so the targets shapes are the one-utterance ones: the double class's
		// chunk of 56 (156 016 B), the float class's of 60 or 52 by the batch (87 632 / 78 896 B).
		const M5Shape m = m5_shape_of(float_class, index, targets);
		const size_t lds = targets ? (float_class ? (index == 1 ? m5_lds_bytes<true, 1, true>() : m5_lds_bytes<true, 0, true>())
		                                          : (index == 1 ? m5_lds_bytes<false, 1, true>() : m5_lds_bytes<false, 0, true>()))
		                           : float_class ? synth5_float_lds_bytes(index) : (index == 1 ? m5_lds_bytes<false, 1>() : m5_lds_bytes<false, 0>());
		const LaunchShape s{m.rows, 0, lds, index + 1, m.rows * m.groups_per_cu};
		return fits(s) ? s : LaunchShape{};
	}
	// utterances per workgroup = DPP rows used by the serial wavefronts.  One row keeps the most
	// workgroups in flight (best latency for small batches); more rows amortise the serial
	// instruction streams once there are more utterances than compute units.
	int rows = forced_rows;
	if (rows != 1 && rows != 2 && rows != 4 && rows != 8) {
		rows = batch > 512 ? 4 : (batch > 256 ? 2 : 1);
		// (fp64 used to stop at two rows: with the compact records four fit with a chunk of 32 and run faster)
		// mixed with SectionDelay 3 or 4 (deeper fp64 delay lines per lane): measured 3.36 vs 2.63 and 2.07 vs 1.65 G samples/s
		if (precision != GVTM_PRECISION_F32 && voices[0].k.section_delay >= 3 && rows > 2) rows = 2;
	}
	// eight rows (two wavefronts per serial role) fit in float only, and the voice variant has the product's shapes only
	if (rows > 4 && (precision != GVTM_PRECISION_F32 || several_voices)) rows = 4;
	// the LDS holds the stream's ring (one for all shapes) or the longest ring of the voices; a shape it does not fit
	// (a down-sampling voice carries the reference's 1024-sample ring per row) gives way to the next smaller one
	for (;; rows /= 2) {
		int ring = stream_ring;
		for (int v = 0; !stream_ring && v < n_voices; ++v) ring = std::max(ring, shape_of_rows(voices[v].k, precision, rows, 0).ring);
		const LaunchShape s = shape_of_rows(voices[0].k, precision, rows, ring);
		if (s.rows == 0 || fits(s)) return s;
		if (s.rows == 1) return LaunchShape{};
		rows = s.rows;
	}
}

// The row map of a launch of several voices, on the device (the launch stays enqueue-only): a stable counting sort of the
// utterances by voice, each voice's list padded to a multiple of `rows`.  One workgroup; thread t takes a contiguous
// stretch of the ids and counts it per voice into column t of a.counts, a scan per voice over the columns (in thread
// order, so that the sort is stable) turns the counts into first slots, and a second walk over the stretch scatters.
// An id outside [0, n_voices) is left out of the map: its utterance gets out_counts = -1, maxabs = 0.
constexpr int kGroupThreads = kGroupVoicesThreads;
__global__ __launch_bounds__(kGroupThreads) void vtm_group_voices_kernel(const GroupVoicesArgs a)
{
	constexpr int T = kGroupThreads;
	__shared__ int scan[T];
	const int t = threadIdx.x;
	const size_t per = (a.batch + T - 1) / T;
	const size_t lo = static_cast<size_t>(t) * per < a.batch ? static_cast<size_t>(t) * per : a.batch;
	const size_t hi = lo + per < a.batch ? lo + per : a.batch;
	int* const cnt = a.counts + t; // cnt[v * T]: utterances of voice v in my stretch, then my first slot for voice v
	for (int v = 0; v < a.n_voices; ++v) cnt[static_cast<size_t>(v) * T] = 0;
	for (size_t i = lo; i < hi; ++i) {
		const int v = a.voice_ids[i];
		if (v >= 0 && v < a.n_voices) {
			++cnt[static_cast<size_t>(v) * T];
		} else {
			if (a.out_counts) a.out_counts[i] = -1;
			if (a.maxabs) a.maxabs[i] = 0.0f;
		}
	}
	for (size_t i = t; i < a.groups * static_cast<size_t>(a.rows); i += T) a.row_map[i] = -1;
	for (size_t g = t; g < a.groups; g += T) a.group_voice[g] = -1;
	__syncthreads();
	size_t first_group = 0;
	for (int v = 0; v < a.n_voices; ++v) {
		const int mine = cnt[static_cast<size_t>(v) * T];
		scan[t] = mine;
		__syncthreads();
		for (int off = 1; off < T; off <<= 1) {
			const int x = t >= off ? scan[t - off] : 0;
			__syncthreads();
			scan[t] += x;
			__syncthreads();
		}
		const size_t total = static_cast<size_t>(scan[T - 1]);
		cnt[static_cast<size_t>(v) * T] = static_cast<int>(first_group * a.rows) + scan[t] - mine;
		const size_t n_groups = (total + a.rows - 1) / a.rows;
		for (size_t g = t; g < n_groups; g += T) a.group_voice[first_group + g] = v;
		first_group += n_groups;
		__syncthreads();
	}
	for (size_t i = lo; i < hi; ++i) {
		const int v = a.voice_ids[i];
		if (v >= 0 && v < a.n_voices) a.row_map[cnt[static_cast<size_t>(v) * T]++] = static_cast<int>(i);
	}
}

hipError_t launch_group_voices(const GroupVoicesArgs& args, hipStream_t stream)
{
	hipLaunchKernelGGL(vtm_group_voices_kernel, dim3(1), dim3(kGroupThreads), 0, stream, args);
	return hipGetLastError();
}

hipError_t launch_synth5(const SynthArgs& args, size_t batch, int precision, int index, hipStream_t stream)
{
	if (!args.k5const || (index != 0 && index != 1)) return hipErrorInvalidValue;
	// (the targets variants live in vtm_kernels_m5t.hip and vtm_kernels_m5ft.hip: one voice, one-shot or a stream's; under
	// several voices in vtm_kernels_m5tv.hip and vtm_kernels_m5ftv.hip: one-shot, the one-utterance shapes)
	if (args.tg_offsets && args.row_map) {
		if (precision == GVTM_PRECISION_F32) return launch_synth5_float_targets_voices(args, batch, index, stream);
		return index == 0 ? launch_synth5_targets_voices(args, batch, stream) : hipErrorInvalidValue;
	}
	if (args.tg_offsets) {
		return precision == GVTM_PRECISION_F32 ? launch_synth5_float_targets(args, batch, index, stream) : launch_synth5_targets(args, batch, index, stream);
	}
	// (the float class lives in vtm_kernels_m5f.hip, as the voice variant does in vtm_kernels_m5v.hip, and the float class's
	// voice variant in vtm_kernels_m5fv.hip)
	if (precision == GVTM_PRECISION_F32) {
		if (!args.row_map) return launch_synth5_float(args, batch, index, stream);
		if (!args.group_voice) return hipErrorInvalidValue;
		return launch_synth5_float_voices(args, batch, index, stream);
	}
	// (the voice variant lives in vtm_kernels_m5v.hip: this file's code object keeps the single-voice kernels only)
	if (!args.row_map) {
		if (index == 1) return launch_synth5_shape<false, 1>(args, batch, stream);
		return launch_synth5_shape<false, 0>(args, batch, stream);
	}
	if (!args.group_voice || index != 0) return hipErrorInvalidValue;
	return launch_synth5_voices(args, batch, stream);
}

hipError_t launch_normalize(const NormalizeArgs& args, size_t batch, hipStream_t stream)
{
	const unsigned bx = static_cast<unsigned>((args.audio_stride + 256 * 8 - 1) / (256 * 8));
	hipLaunchKernelGGL(vtm_normalize_kernel, dim3(bx > 0 ? bx : 1, static_cast<unsigned>(batch)), dim3(256), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
