// Streams that listen (include/gama_vtm.h, "Streams that listen"): the analysis ring of the editor's interactive window
// (InteractiveAudio.cpp:146-158, 192-205: every output sample goes into a ring of 65 536; AnalysisWindow.cpp:199-225: the
// window reads the ring whenever it is full), one per utterance of a stream, on the device.
//
// The rule.  An utterance's samples since the stream's last reset are numbered from 0 in the order the pushes and the finish
// return them; buffer k is the samples [65536 k, 65536 (k + 1)); a buffer is analysed by the launch that brings its last
// sample; an incomplete ring is never analysed.  This header is the one text of that arithmetic for the host (which knows
// every sample count before a launch) and of the ragged copy that moves a launch's samples between its audio rows and the
// rings (vtm_listen.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/gama_vtm.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GVTM_LISTEN_HD __host__ __device__ inline
#else
#define GVTM_LISTEN_HD inline
#endif

namespace gvtm {

constexpr int64_t kListenRing = GVTM_ANALYSIS_FFT_SIZE;

// the buffers that n_new more samples complete on a ring holding `fill`, and what the ring holds afterwards; a fill outside
// [0, 65536) or a negative n_new completes nothing and leaves the fill
GVTM_LISTEN_HD int64_t listen_buffer_count(int64_t fill, int64_t n_new, int64_t* fill_after)
{
	if (fill < 0 || fill >= kListenRing || n_new < 0) {
		if (fill_after) *fill_after = fill;
		return 0;
	}
	const int64_t total = fill + n_new;
	if (fill_after) *fill_after = total % kListenRing;
	return total / kListenRing;
}

// What a launch that brings n samples to a ring holding `fill` does, K = listen_buffer_count(fill, n):
//   head    the row's first head_len samples go to ring[fill ..)
//   ring    K >= 1: the ring is full and is analysed where it lies (buffer 0 of the launch)
//   inside  K >= 2: the buffers 1 .. K - 1 are analysed in the audio row, from sample inside_first on
//   tail    K >= 1: the row's tail_len samples behind its last complete buffer, from tail_src on, go to ring[0 ..)
struct ListenMove {
	int64_t buffers, fill_after;
	int64_t head_len;
	int64_t inside_first;
	int64_t tail_src, tail_len;
};

GVTM_LISTEN_HD ListenMove listen_move(int64_t fill, int64_t n)
{
	ListenMove m{};
	m.buffers = listen_buffer_count(fill, n, &m.fill_after);
	const int64_t room = kListenRing - fill;
	m.head_len = n < room ? n : room;
	m.inside_first = room;
	if (m.buffers >= 1) {
		m.tail_src = room + (m.buffers - 1) * kListenRing;
		m.tail_len = n - m.tail_src; // (= fill_after)
	}
	return m;
}

#if defined(__HIP__)

// A ragged copy of float rows: utterance b's len[b] samples from src + b * src_stride + src_off[b] to dst + b * dst_stride +
// dst_off[b]; any of the three may be 0 or odd, and no row base is aligned.  The tables are on the device; max_len, the
// largest length, sizes the grid.  src and dst do not overlap.
struct ListenCopyArgs {
	const float* src;
	size_t src_stride;
	float* dst;
	size_t dst_stride;
	const int64_t* src_off;   // [batch]
	const int64_t* dst_off;   // [batch]
	const int64_t* len;       // [batch]
	size_t batch;
};

hipError_t launch_listen_copy(const ListenCopyArgs& args, int64_t max_len, hipStream_t stream);

#endif

} // namespace gvtm
