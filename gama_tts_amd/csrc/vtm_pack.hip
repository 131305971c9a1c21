// CDNA4 (gfx950) copy kernels of the packed host entries (gvtm_synthesize_packed_host*): the batch crosses PCIe packed,
// utterances back to back, and the synthesis kernels read and write padded rows, so each slice is unpacked in front of
// its synthesis launch and packed again behind it.
//
//   vtm_unpack_frames_kernel   packed frames -> [n][max_frames][16] rows, and the slice's int32 frame counts
//   vtm_pack_samples_kernel    [n][audio_stride] float rows -> the packed output, float32 unscaled or int16 scaled and
//                              rounded exactly as vtm_normalize_kernel does; the gap up to the next utterance is zeros
//
// Both are HBM-bound element-wise passes: every lane moves 16 bytes per load and per store.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vtm_pack.hpp"

namespace gvtm {

// grid (blocks over the longest row, utterances); a frame is four 16-byte items
__global__ __launch_bounds__(kPackThreads) void vtm_unpack_frames_kernel(const UnpackFramesArgs a)
{
	const int64_t base = a.frame_offsets[0];
	for (size_t b = blockIdx.y; b < a.n; b += gridDim.y) {
		const int64_t first = a.frame_offsets[b];
		int64_t frames = a.frame_offsets[b + 1] - first;
		// (the host has checked the tables; a row never takes more than it holds)
		frames = frames < 0 ? 0 : frames > static_cast<int64_t>(a.max_frames) ? static_cast<int64_t>(a.max_frames) : frames;
		if (blockIdx.x == 0 && threadIdx.x == 0) a.frame_counts[b] = static_cast<int32_t>(frames);
		const float4* __restrict__ in = reinterpret_cast<const float4*>(a.packed) + (first - base) * 4;
		float4* __restrict__ out = reinterpret_cast<float4*>(a.padded) + b * a.max_frames * 4;
		const int64_t items = frames * 4;
		for (int64_t i = static_cast<int64_t>(blockIdx.x) * kPackThreads + threadIdx.x; i < items; i += static_cast<int64_t>(gridDim.x) * kPackThreads) {
			out[i] = in[i];
		}
	}
}

// WAVEFileWriter::writeSample's rounding of a scaled sample (vtm_normalize_kernel: the same two products, each rounded)
__device__ __forceinline__ unsigned pcm16_bits(float x, float scale)
{
	const float v = x * scale;
	return static_cast<unsigned>(static_cast<uint16_t>(static_cast<int16_t>(static_cast<int>(roundf(v * 32767.0f)))));
}

// grid (blocks over the longest extent, utterances); a lane takes a group of 8 samples: starts and extents are multiples of 8
__global__ __launch_bounds__(kPackThreads) void vtm_pack_samples_kernel(const PackSamplesArgs a)
{
	const int64_t base = a.sample_offsets[0];
	for (size_t b = blockIdx.y; b < a.n; b += gridDim.y) {
		const int64_t start = a.sample_offsets[b] - base;
		int64_t extent = a.sample_offsets[b + 1] - a.sample_offsets[b];
		extent = extent > static_cast<int64_t>(a.audio_stride) ? static_cast<int64_t>(a.audio_stride) : extent; // (never: the host sized the rows)
		int64_t count = a.counts[b];
		count = count < 0 ? 0 : count > extent ? extent : count;
		const float peak = a.maxabs[b];
		const float scale = (peak < 1.0e-30f) ? 0.0f : 0.95f / peak;
		if (a.scales && blockIdx.x == 0 && threadIdx.x == 0) a.scales[b] = scale;
		const float* __restrict__ row = a.audio + b * a.audio_stride;
		for (int64_t g = static_cast<int64_t>(blockIdx.x) * kPackThreads + threadIdx.x; 8 * g < extent; g += static_cast<int64_t>(gridDim.x) * kPackThreads) {
			const int64_t i = 8 * g;
			const float4 lo = *reinterpret_cast<const float4*>(row + i);
			const float4 hi = *reinterpret_cast<const float4*>(row + i + 4);
			float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
			// the last group of an utterance carries the zeros of the gap (the row itself is defined up to its count only)
#pragma unroll
			for (int q = 0; q < 8; ++q) x[q] = i + q < count ? x[q] : 0.0f;
			if (a.out_f32) {
				float4* out = reinterpret_cast<float4*>(a.out_f32 + start + i);
				out[0] = make_float4(x[0], x[1], x[2], x[3]);
				out[1] = make_float4(x[4], x[5], x[6], x[7]);
			} else {
				unsigned w[4];
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					const unsigned s0 = i + 2 * q < count ? pcm16_bits(x[2 * q], scale) : 0u;
					const unsigned s1 = i + 2 * q + 1 < count ? pcm16_bits(x[2 * q + 1], scale) : 0u;
					w[q] = s0 | (s1 << 16);
				}
				*reinterpret_cast<uint4*>(a.out_i16 + start + i) = make_uint4(w[0], w[1], w[2], w[3]);
			}
		}
	}
}

namespace {

unsigned blocks_over(size_t items)
{
	const size_t blocks = (items + kPackThreads - 1) / kPackThreads;
	return static_cast<unsigned>(blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks); // (the kernels stride over what is left)
}

} // namespace

hipError_t launch_unpack_frames(const UnpackFramesArgs& args, hipStream_t stream)
{
	if (args.n == 0) return hipSuccess;
	const unsigned by = static_cast<unsigned>(args.n < kPackMaxGridY ? args.n : kPackMaxGridY);
	hipLaunchKernelGGL(vtm_unpack_frames_kernel, dim3(blocks_over(args.max_frames * 4), by), dim3(kPackThreads), 0, stream, args);
	return hipGetLastError();
}

hipError_t launch_pack_samples(const PackSamplesArgs& args, hipStream_t stream)
{
	if (args.n == 0) return hipSuccess;
	if ((args.out_f32 == nullptr) == (args.out_i16 == nullptr)) return hipErrorInvalidValue;
	const unsigned by = static_cast<unsigned>(args.n < kPackMaxGridY ? args.n : kPackMaxGridY);
	hipLaunchKernelGGL(vtm_pack_samples_kernel, dim3(blocks_over(args.audio_stride / 8), by), dim3(kPackThreads), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
