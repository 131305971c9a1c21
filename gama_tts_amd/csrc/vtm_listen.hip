// The ragged copy of a listening stream (vtm_listen.hpp; gfx950): a launch's samples from its audio rows into the analysis
// rings, and what lies behind the last complete buffer back to the rings' fronts.
//   listen_copy_kernel   grid (chunks of 4096 samples, utterances); a workgroup of 256 copies one chunk of one utterance's
//                        run.  Where source and destination agree modulo 16 bytes: up to three samples peeled to the
//                        destination's 16-byte boundary, then 16-byte loads and stores, consecutive lanes on consecutive
//                        addresses, four per thread in flight, then up to three samples behind (peel and rest are chunk 0's).
//                        Where they do not agree: 4-byte loads and stores, sixteen per thread.  The row bases are the
//                        caller's (audio_stride), so which of the two holds is only known here.
// A workgroup whose chunk lies behind its utterance's length exits; utterances beyond the grid's y limit are reached by a
// stride over y.
#include "vtm_listen.hpp"

namespace gvtm {

namespace {

constexpr unsigned kCopyThreads = 256;
constexpr unsigned kCopyPerThread = 4;                                   // 16-byte accesses per thread
constexpr unsigned kCopyVectors = kCopyThreads * kCopyPerThread;         // per chunk
constexpr unsigned kCopyChunk = 4 * kCopyVectors;                        // samples per chunk: 4096
constexpr unsigned kCopyMaxY = 65535;

__global__ __launch_bounds__(kCopyThreads) void listen_copy_kernel(const ListenCopyArgs a)
{
	const unsigned tid = threadIdx.x;
	const int64_t chunk = blockIdx.x;
	for (size_t b = blockIdx.y; b < a.batch; b += gridDim.y) {
		const int64_t n = a.len[b];
		if (n <= 0 || chunk * kCopyChunk >= n) continue;
		const float* s = a.src + b * a.src_stride + a.src_off[b];
		float* d = a.dst + b * a.dst_stride + a.dst_off[b];
		const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
		if (((sa ^ da) & 15) == 0) {
			// (both are float addresses: the distance to the boundary is a whole number of samples)
			int64_t peel = static_cast<int64_t>(((16 - (da & 15)) & 15) / 4);
			if (peel > n) peel = n;
			const int64_t vectors = (n - peel) / 4, rest = n - peel - 4 * vectors;
			if (chunk == 0) {
				if (tid < peel) d[tid] = s[tid];
				if (tid < rest) d[peel + 4 * vectors + tid] = s[peel + 4 * vectors + tid];
			}
			const float4* s4 = reinterpret_cast<const float4*>(s + peel);
			float4* d4 = reinterpret_cast<float4*>(d + peel);
			float4 v[kCopyPerThread];
#pragma unroll
			for (unsigned j = 0; j < kCopyPerThread; ++j) {
				const int64_t i = chunk * kCopyVectors + j * kCopyThreads + tid;
				if (i < vectors) v[j] = s4[i];
			}
#pragma unroll
			for (unsigned j = 0; j < kCopyPerThread; ++j) {
				const int64_t i = chunk * kCopyVectors + j * kCopyThreads + tid;
				if (i < vectors) d4[i] = v[j];
			}
		} else {
			float v[4 * kCopyPerThread];
#pragma unroll
			for (unsigned j = 0; j < 4 * kCopyPerThread; ++j) {
				const int64_t i = chunk * kCopyChunk + j * kCopyThreads + tid;
				if (i < n) v[j] = s[i];
			}
#pragma unroll
			for (unsigned j = 0; j < 4 * kCopyPerThread; ++j) {
				const int64_t i = chunk * kCopyChunk + j * kCopyThreads + tid;
				if (i < n) d[i] = v[j];
			}
		}
	}
}

} // namespace

hipError_t launch_listen_copy(const ListenCopyArgs& args, int64_t max_len, hipStream_t stream)
{
	if (args.batch == 0 || max_len <= 0) return hipSuccess;
	const int64_t chunks = (max_len + kCopyChunk - 1) / kCopyChunk;
	if (chunks > 0x7fffffff) return hipErrorInvalidValue;
	const unsigned y = static_cast<unsigned>(args.batch < kCopyMaxY ? args.batch : kCopyMaxY);
	hipLaunchKernelGGL(listen_copy_kernel, dim3(static_cast<unsigned>(chunks), y), dim3(kCopyThreads), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
