// Lengths to offsets, for the kernels that pack one list per utterance back to back behind a counting pass
// (vtm_intonation.hip, vtm_rules.hip): one workgroup of kScanThreads threads over the batch.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace gvtm {

constexpr int kScanThreads = 1024;

// offsets[1 ..= batch] hold the lengths; they leave as the ends of the lists laid back to back, offsets[0] = 0.  A list that
// would end beyond `capacity` is dropped (length 0, status[utt] = no_room where status is not null), so the sums behind it
// do not count it: 1024 lengths at a time are summed in parallel, and only a block in which a list does not fit is walked
// one by one.  To be called by every thread of a workgroup of kScanThreads.
__device__ __forceinline__ void lengths_to_offsets(int64_t* offsets, size_t batch, int64_t capacity, int32_t* status, int32_t no_room)
{
	__shared__ int64_t sums[2][kScanThreads];
	__shared__ int64_t running; // the end of the lists in front of this block of lengths
	const int t = threadIdx.x;
	if (t == 0) {
		running = 0;
		offsets[0] = 0;
	}
	for (size_t block = 0; block < batch; block += kScanThreads) {
		const size_t utt = block + t;
		const bool mine = utt < batch;
		int64_t length = mine ? offsets[utt + 1] : 0;
		if (length < 0) length = 0;
		sums[0][t] = length;
		__syncthreads(); // (also: `running` of the block before is written)
		const int64_t start = running;
		int from = 0;
		for (int step = 1; step < kScanThreads; step <<= 1) { // inclusive sums, doubling
			sums[from ^ 1][t] = sums[from][t] + (t >= step ? sums[from][t - step] : 0);
			from ^= 1;
			__syncthreads();
		}
		int64_t end = start + sums[from][t];
		const bool all_fit = start + sums[from][kScanThreads - 1] <= capacity; // the same for every thread
		__syncthreads(); // every thread has read `running` and the block's total
		if (all_fit) {
			if (t == kScanThreads - 1) running = end;
		} else {
			// a list of this block does not fit: one thread lays the block out, list by list
			sums[0][t] = length;
			__syncthreads();
			if (t == 0) {
				int64_t at = start;
				for (int i = 0; i < kScanThreads; ++i) {
					const int64_t len = sums[0][i];
					const bool fits = at + len <= capacity;
					if (fits) at += len;
					sums[0][i] = fits ? at : -at - 1; // the list's end, or (dropped) the end before it, marked
				}
				running = at;
			}
			__syncthreads();
			end = sums[0][t];
			if (end < 0) {
				end = -end - 1;
				if (mine && status) status[utt] = no_room;
			}
		}
		if (mine) offsets[utt + 1] = end;
		__syncthreads(); // `running` is written, sums may be overwritten
	}
}

} // namespace gvtm
