// Launch interface of the packed host entries' two copy kernels (vtm_pack.hip): packed frames -> the padded rows the
// synthesis kernels read, and the padded sample rows -> the packed output (include/gama_vtm.h, "Ragged batches").
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace gvtm {

constexpr int kPackThreads = 256;
constexpr unsigned kPackMaxGridY = 65535; // utterances beyond it are taken by the same workgroups in a second round

// One slice of n utterances.  The offset tables are the batch's, on the device, pointing at the slice's first entry:
// utterance b of the slice owns the frames [frame_offsets[b], frame_offsets[b + 1]), and `packed` starts at frame
// frame_offsets[0].
struct UnpackFramesArgs {
	const float* packed;          // [frames of the slice][16], 16-byte aligned
	const int64_t* frame_offsets; // [n + 1]
	float* padded;                // [n][max_frames][16] out, 16-byte aligned; rows are not written beyond their count
	int32_t* frame_counts;        // [n] out
	size_t n, max_frames;
};

// Utterance b leaves at out + (sample_offsets[b] - sample_offsets[0]) and fills its extent up to sample_offsets[b + 1]:
// counts[b] samples, then zeros.  Every offset is a multiple of 8 samples, and so is audio_stride.
struct PackSamplesArgs {
	const float* audio;            // [n][audio_stride], 32-byte aligned; a row is defined up to its count only
	const int64_t* counts;         // [n] samples the synthesis launch reported
	const float* maxabs;           // [n]
	const int64_t* sample_offsets; // [n + 1]
	float* out_f32;                // unscaled samples, or null
	int16_t* out_i16;              // or null: scaled by 0.95 / max|x| and rounded as vtm_normalize_kernel does
	float* scales;                 // [n] out (int16 only), or null
	size_t n, audio_stride;
};

hipError_t launch_unpack_frames(const UnpackFramesArgs& args, hipStream_t stream);
hipError_t launch_pack_samples(const PackSamplesArgs& args, hipStream_t stream);

} // namespace gvtm
