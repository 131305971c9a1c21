// Spectrum analysis kernels (vtm_analysis.hpp holds the rule and the butterflies; gfx950):
//   analysis_count_kernel   step 4 for every utterance: buffers_out
//   analysis_peak_kernel    one workgroup of 1024 per buffer: the peak over its 65 536 samples (coalesced 16-byte loads where
//                           the buffer is 16-byte aligned, 4-byte loads where not), the wavefront maximum by DPP row
//                           rotations and one LDS atomic per row; then normCoef to the slot's scratch and, with a signal
//                           output, the first W normalised samples (the second read of the buffer hits L2)
//   analysis_pass_a_kernel  8 workgroups per buffer: 16 columns of the 128 x 256 split each, normalised and windowed on the
//                           way in, four radix-4 steps between two LDS images of 32 KB, the last one straight to T
//   analysis_pass_b_kernel  8 workgroups per buffer: 32 rows each, T in (padded image: 33 KB each), three radix-4 steps and a
//                           radix-2 step, the last one straight to Z
//   analysis_pass_c_kernel  one thread per bin below n_bins: untangling, magnitude, 1/256, log and floor
// T and Z are the slot's scratch (256 KB each); between two passes they stay in L2 / the Infinity Cache.
// Every kernel works out for itself whether its pair (utterance, buffer) exists, from the counts on the device, so the
// host never reads them.
#include "vtm_analysis.hpp"

namespace gvtm {

namespace {

constexpr unsigned kPeakThreads = 1024;

// DPP row rotate: lane i of a 16-lane row receives lane (i - N) mod 16
template <int N>
__device__ __forceinline__ float row_rotate(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xF, 0xF, true));
}

// the buffers of utterance b (step 4), its count cut at the row's length
__device__ __forceinline__ int64_t utterance_buffers(const AnalysisArgs& a, size_t b, int64_t& first)
{
	first = a.first ? a.first[b] : 0;
	int64_t count = a.counts[b];
	if (count > static_cast<int64_t>(a.audio_stride)) count = static_cast<int64_t>(a.audio_stride);
	return analysis_buffer_count(count, first, static_cast<int64_t>(a.max_buffers));
}

// The pair of slot `slot` of this launch: false if it lies behind the batch or behind its utterance's buffers; else its
// row of the outputs (its number, or with a slot table its place in the utterance's block) and its samples.
__device__ __forceinline__ bool slot_pair(const AnalysisArgs& a, size_t slot, size_t& row, const float*& samples)
{
	const size_t pair = a.first_pair + slot;
	// (a batch has fewer than 2^31 pairs: 32-bit division)
	const size_t b = static_cast<unsigned>(pair) / static_cast<unsigned>(a.max_buffers), k = static_cast<unsigned>(pair) % static_cast<unsigned>(a.max_buffers);
	if (b >= a.batch) return false;
	int64_t first;
	if (static_cast<int64_t>(k) >= utterance_buffers(a, b, first)) return false;
	samples = a.audio + b * a.audio_stride + static_cast<size_t>(first) + k * static_cast<size_t>(kAnalysisSize);
	row = a.out_slots ? b * a.out_stride + static_cast<size_t>(a.out_slots[b]) + k : pair;
	return true;
}

__global__ void analysis_count_kernel(const AnalysisArgs a)
{
	const size_t b = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (b >= a.batch) return;
	int64_t first;
	a.buffers_out[b] = static_cast<int32_t>(utterance_buffers(a, b, first));
}

__global__ __launch_bounds__(kPeakThreads) void analysis_peak_kernel(const AnalysisArgs a)
{
	__shared__ unsigned peak_bits;
	size_t pair;
	const float* s;
	if (!slot_pair(a, blockIdx.x, pair, s)) return; // (the whole workgroup)
	const unsigned tid = threadIdx.x;
	if (tid == 0) peak_bits = 0;
	__syncthreads();
	float mx = 0.0f;
	if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
		const float4* s4 = reinterpret_cast<const float4*>(s);
#pragma unroll 8
		for (unsigned j = 0; j < kAnalysisSize / 4 / kPeakThreads; ++j) {
			const float4 v = s4[tid + j * kPeakThreads];
			mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
		}
	} else {
#pragma unroll 8
		for (unsigned j = 0; j < kAnalysisSize / kPeakThreads; ++j) mx = fmaxf(mx, fabsf(s[tid + j * kPeakThreads]));
	}
	// by 15, 14, 12 and 8 a lane takes in the lanes i + 1, i + 2, i + 4 and i + 8 of its row: the row's first lane ends up
	// with the row's maximum.  (Not negative, so the order of the bits is the order of the floats; fmaxf drops a NaN, as the
	// reference's `absValue > maxValue` does.)
	mx = fmaxf(mx, row_rotate<15>(mx));
	mx = fmaxf(mx, row_rotate<14>(mx));
	mx = fmaxf(mx, row_rotate<12>(mx));
	mx = fmaxf(mx, row_rotate<8>(mx));
	if ((tid & 15) == 0) atomicMax(&peak_bits, __float_as_uint(mx));
	__syncthreads();
	const float coef = analysis_norm_coef(__uint_as_float(peak_bits));
	if (tid == 0) a.norm_coefs[blockIdx.x] = coef;
	if (a.signal) {
		float* out = a.signal + pair * a.W;
		for (unsigned i = tid; i < a.W; i += kPeakThreads) out[i] = analysis_normalised(s[i], coef);
	}
}

__global__ __launch_bounds__(kAnalysisThreads) void analysis_pass_a_kernel(const AnalysisArgs a)
{
	__shared__ AnalysisComplex u[kAnalysisImage], v[kAnalysisImage];
	const size_t slot = blockIdx.x / kAnalysisGroupsA;
	const unsigned g = blockIdx.x % kAnalysisGroupsA;
	size_t pair;
	const float* s;
	if (!slot_pair(a, slot, pair, s)) return;
	const float coef = a.norm_coefs[slot];
	const bool aligned8 = (reinterpret_cast<uintptr_t>(s) & 7) == 0;
	AnalysisComplex* T = a.T + slot * kAnalysisHalf;
	const unsigned tid = threadIdx.x;
	analysis_pass_a<0>(tid, g, s, coef, a.window, a.W, aligned8, a.table, u, v, T);
	__syncthreads();
	analysis_pass_a<1>(tid, g, s, coef, a.window, a.W, aligned8, a.table, u, v, T);
	__syncthreads();
	analysis_pass_a<2>(tid, g, s, coef, a.window, a.W, aligned8, a.table, u, v, T);
	__syncthreads();
	analysis_pass_a<3>(tid, g, s, coef, a.window, a.W, aligned8, a.table, u, v, T);
	__syncthreads();
	analysis_pass_a<4>(tid, g, s, coef, a.window, a.W, aligned8, a.table, u, v, T);
}

__global__ __launch_bounds__(kAnalysisThreads) void analysis_pass_b_kernel(const AnalysisArgs a)
{
	__shared__ AnalysisComplex u[kAnalysisImagePadded], v[kAnalysisImagePadded];
	const size_t slot = blockIdx.x / kAnalysisGroupsB;
	const unsigned h = blockIdx.x % kAnalysisGroupsB;
	size_t pair;
	const float* s;
	if (!slot_pair(a, slot, pair, s)) return;
	const AnalysisComplex* T = a.T + slot * kAnalysisHalf;
	AnalysisComplex* Z = a.Z + slot * kAnalysisHalf;
	const unsigned tid = threadIdx.x;
	analysis_pass_b<0>(tid, h, T, a.table, u, v, Z);
	__syncthreads();
	analysis_pass_b<1>(tid, h, T, a.table, u, v, Z);
	__syncthreads();
	analysis_pass_b<2>(tid, h, T, a.table, u, v, Z);
	__syncthreads();
	analysis_pass_b<3>(tid, h, T, a.table, u, v, Z);
	__syncthreads();
	analysis_pass_b<4>(tid, h, T, a.table, u, v, Z);
}

__global__ __launch_bounds__(kAnalysisThreads) void analysis_pass_c_kernel(const AnalysisArgs a, unsigned groups_per_buffer)
{
	const size_t slot = blockIdx.x / groups_per_buffer;
	const unsigned k = (blockIdx.x % groups_per_buffer) * kAnalysisThreads + threadIdx.x;
	size_t pair;
	const float* s;
	if (!slot_pair(a, slot, pair, s)) return;
	if (k >= a.n_bins) return;
	const AnalysisComplex x = analysis_untangle(a.Z + slot * kAnalysisHalf, a.table, k);
	a.spectra[pair * a.n_bins + k] = analysis_level(analysis_magnitude(x), a.log_scale, a.min_db);
}

} // namespace

hipError_t launch_analysis(const AnalysisArgs& args, hipStream_t stream)
{
	if (args.buffers_out && args.first_pair == 0 && args.batch > 0) {
		hipLaunchKernelGGL(analysis_count_kernel, dim3(static_cast<unsigned>((args.batch + 255) / 256)), dim3(256), 0, stream, args);
	}
	if (args.n_pairs == 0) return hipGetLastError();
	const unsigned n = static_cast<unsigned>(args.n_pairs);
	hipLaunchKernelGGL(analysis_peak_kernel, dim3(n), dim3(kPeakThreads), 0, stream, args);
	if (args.spectra) {
		const unsigned groups_c = (args.n_bins + kAnalysisThreads - 1) / kAnalysisThreads;
		hipLaunchKernelGGL(analysis_pass_a_kernel, dim3(n * kAnalysisGroupsA), dim3(kAnalysisThreads), 0, stream, args);
		hipLaunchKernelGGL(analysis_pass_b_kernel, dim3(n * kAnalysisGroupsB), dim3(kAnalysisThreads), 0, stream, args);
		hipLaunchKernelGGL(analysis_pass_c_kernel, dim3(n * groups_c), dim3(kAnalysisThreads), 0, stream, args, groups_c);
	}
	return hipGetLastError();
}

} // namespace gvtm
