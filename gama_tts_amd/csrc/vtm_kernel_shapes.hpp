// The shapes of vtm_synth_kernel and the one function that launches them, for the translation units that hold a variant of
// the kernel (vtm_kernels.hip: frames, one voice and several; vtm_kernels_targets.hip: targets; vtm_kernels_targets_voices.hip:
// targets under several voices): included inside namespace gvtm, behind vtm_kernel_v2.inc, whose constants a shape is made of.
// A unit is one launch_v2_variant<FLAGS> call per variant; a new variant is a new unit with one such call.
#pragma once

// ---- kernel shapes ----
//
// A shape is what one vtm_synth_kernel launch is built from: precision <CT, ST>, SectionDelay D, utterances per workgroup
// U (DPP rows), tube layout; and from those the chunk length C, the helper wavefronts NH, the wavefronts per workgroup,
// the ring length and the LDS bytes.  v2_shape() below is the ONE description of it and with_shape() the ONE place where
// a runtime (precision, rows, SectionDelay, layout) becomes template arguments: the launch, the queries of the launch
// interface and synth_launch_shape() all go through them, so they cannot disagree.  A new shape is a new line here.
struct KernelShape { int rows, chunk, helpers, waves; };

template <typename CT, typename ST, int D, int U, int LAYOUT>
constexpr KernelShape v2_shape()
{
	constexpr bool f32 = sizeof(CT) == 4, mixed = sizeof(CT) == 8 && sizeof(ST) == 4, wide = LAYOUT == 1;
	// Chunk length C: a multiple of 4 (scan blocks) and of the tube unroll (2 for SectionDelay 1, D for even D, 6 for 3).
	// Helpers NH: 8 resp. 12 wavefronts per workgroup on the 10 + 6 tube (16 in float with four or eight rows); the
	// 48-section tube's workgroups have U tube wavefronts + 4 other serial ones + helpers = 8 resp. 12 (three wavefronts
	// per SIMD: 168 registers each).
	// LDS per workgroup: tests/tools/lds_sizes.py (float 1x144 120 KB, 2x96 152, 4x48 154; mixed 4x32 154; fp64 4x32 159).
	// (fp64 with several rows: resampler table without its delta half)
	int C = 0, NH = 0;
	switch (U) {
	case 1:
		// the tick time is the tube wavefront's plus what a tick costs besides (barrier, stage prologues): measured
		// on batch 256 in float, C = 60 / 96 / 120 / 144 / 168 / 192 -> 3.73 / 3.58 / 3.53 / 3.48 / 3.52 / 3.59 ms (108 and
		// 180, whose last 64-item helper pass is half empty: 3.73 / 3.70); mixed 60 / 96 / 120 -> 4.19 / 4.04 / 4.15;
		// fp64 60 / 72 / 84 -> 4.14 / 4.65 / 4.07 (LDS ends there).  No power-of-two lengths (LDS strides).
		C = f32 ? 144 : (mixed ? 96 : 84), NH = 3;
		break;
	case 2:
		// U > 1: every tick has fixed costs (barrier, stage prologues, ticket traffic, partly filled 64-item
		// passes), so the longest chunk LDS allows wins: measured on batch 4096 in float, C = 24 / 36 / 48
		// -> 24.8 / 21.6 / 18.4 ms; batch 512, C = 24 / 48 / 96 -> 4.71 / 4.64 / 4.38 ms.
		C = f32 ? 96 : 48, NH = wide ? 6 : 7;
		break;
	case 4:
		// in double: 32 steps = two FULL 64-item passes per stage (24 steps left the second pass half empty and
		// made every pass a large share of a tick); SectionDelay 3 unrolls the tube by 6 and keeps 24.  (28 steps for
		// SectionDelay 1, so that the resampler's 61.6 outputs per chunk fill ONE pass, measured slower: 12.7 vs 13.3 G.)
		// (float, SectionDelay 3: 36 -- reference model 3 down-samples to 44.1 kHz, so its rings are 1024 samples each,
		// and with the lane-indexed tube record 48 steps no longer fit)
		C = f32 ? (D == 3 ? 36 : 48) : (D == 3 ? 24 : 32);
		// Float: ELEVEN helpers = 16 wavefronts, the most a workgroup can have (128 registers each).  With the tube
		// record in blocks of four steps the tube and pre-tube filter wavefronts need 177 / 150 cycles per step and the
		// helper pool is the tick: same box, 4096 utterances, SectionDelay 2 x 2000 frames: 7 / 8 / 9 / 11 helpers
		// -> 107.6 / 106.2 / 103.6 / 100.0 ms; SectionDelay 1 x 500 frames: 14.24 / 14.00 / 13.68 / 13.11 ms.  (Round 2, when
		// the tube was the tick: 14 / 16 wavefronts 63.0 -> 62.6 ms.  The double models spill at 128 registers: fp64 22.8 -> 24.5 ms.)
		NH = wide ? 4 : (f32 ? 11 : 7);
		break;
	case 8:
		// float on the 10 + 6 tube only: two wavefronts per serial role + 6 helpers = 16
		C = 24, NH = 6;
		break;
	}
	return KernelShape{U, C, NH, v2::serial_waves<U, LAYOUT>() + NH};
}

template <typename CT_, typename ST_, int D_, int U_, int LAYOUT_>
struct V2Shape {
	using CT = CT_;
	using ST = ST_;
	static constexpr int D = D_, U = U_, LAYOUT = LAYOUT_;
	static constexpr KernelShape k = v2_shape<CT, ST, D, U, LAYOUT>();
	static constexpr int C = k.chunk, NH = k.helpers, kWaves = k.waves;
	static_assert(U == 1 || U == 2 || U == 4 || (U == 8 && sizeof(CT) == 4 && LAYOUT == 0), "eight rows: float on the 10 + 6 tube only");
	static_assert(LAYOUT == 0 || (LAYOUT == 1 && D == 1), "the 48-lane layout runs with SectionDelay 1");
	static_assert(D >= 1 && D <= kMaxSectionDelay && C > 0 && C % 4 == 0 && C % (D == 3 ? 6 : (D == 1 ? 2 : D)) == 0, "chunk: whole scan blocks and tube unrolls");
	static_assert(kWaves <= 16, "a workgroup has at most 16 wavefronts");
	// (a stream keeps ONE ring length for all shapes, the one-row shape's: longer than this shape needs, never shorter)
	static_assert(C <= v2_shape<CT, ST, D, 1, LAYOUT>().chunk, "a stream's ring, the one-row shape's, holds every shape's chunks");
	// LDS bytes of a workgroup whose internal-rate rings hold xr samples each
	static size_t lds_bytes(int xr) { return v2::smem_bytes<CT, ST, U, C, v2::lane_rec<CT, LAYOUT>()>(xr); }
};

// Calls f(V2Shape<...>{}) for the shape of a runtime (precision, rows, SectionDelay, layout); `refused` where there is none.
// Eight rows exist in float only; the 48-lane layout (VocalTractModel4: 48 section lanes = one utterance per tube
// wavefront) has SectionDelay 1 only and up to four tube wavefronts per workgroup, so more rows become four.
// f must not name the kernel unless it launches it: naming vtm_synth_kernel<...> instantiates it.
template <typename R, typename F>
static R with_shape(int precision, int rows, int delay, int layout, R refused, F f)
{
	const bool wide = layout == 1;
	auto with_delay = [&](auto ct, auto st, auto u) -> R {
		using CT = decltype(ct);
		using ST = decltype(st);
		constexpr int U = decltype(u)::value;
		if (wide) return delay == 1 ? f(V2Shape<CT, ST, 1, (U < 4 ? U : 4), 1>{}) : refused;
		switch (delay) {
		case 1: return f(V2Shape<CT, ST, 1, U, 0>{});
		case 2: return f(V2Shape<CT, ST, 2, U, 0>{});
		case 3: return f(V2Shape<CT, ST, 3, U, 0>{});
		case 4: return f(V2Shape<CT, ST, 4, U, 0>{});
		}
		return refused;
	};
	auto with_rows = [&](auto ct, auto st) -> R {
		if constexpr (sizeof(ct) == 4) {
			if (rows == 8) return with_delay(ct, st, std::integral_constant<int, 8>{});
		}
		switch (rows) {
		case 4: return with_delay(ct, st, std::integral_constant<int, 4>{});
		case 2: return with_delay(ct, st, std::integral_constant<int, 2>{});
		case 1: return with_delay(ct, st, std::integral_constant<int, 1>{});
		}
		return refused;
	};
	switch (precision) {
	case GVTM_PRECISION_F32: return with_rows(float{}, float{});
	case GVTM_PRECISION_MIXED: return with_rows(double{}, float{});
	case GVTM_PRECISION_F64: return with_rows(double{}, double{});
	}
	return refused;
}

// internal-rate ring of a workgroup row (vtm_design.hpp: synth_ring_for)
static int ring_length(const DeviceConstants& k, int chunk)
{
	return synth_ring_for(k.upsampling, k.pad, chunk);
}

// ---- the launch ----
//
// The ONE launch of a shape S in a variant of vtm_synth_kernel.  FLAGS: a subset of v2::kVoicesFlag | v2::kTargetsFlag, OR-ed
// into the kernel's last template argument.  `work`: utterances (one workgroup per S::U of them), or with the voices flag the
// workgroups of launch_group_voices' map; args.xr is then the longest ring of the launch's voices (what the LDS is sized for;
// a stream's: of the voices' stream rings, which args.stream_chunk fixes).
// Eight rows are a diagnostics build's forced shape and the plain frames variant's alone: every other variant refuses them
// without naming the kernel, so its code object holds the product's shapes only.
template <typename S, int FLAGS>
static hipError_t launch_v2(const SynthArgs& args, size_t work, hipStream_t stream)
{
	constexpr bool VOICES = (FLAGS & v2::kVoicesFlag) != 0;
	if constexpr (FLAGS != 0 && S::U == 8) {
		return hipErrorInvalidValue;
	} else {
		auto fn = v2::vtm_synth_kernel<typename S::CT, typename S::ST, S::D, S::U, S::C, S::NH, S::LAYOUT | FLAGS>;
		if (args.xr < ring_length(args.k, S::C) || (args.xr & (args.xr - 1)) != 0 || 2 * S::C + 4 * args.k.pad + 64 > args.xr) return hipErrorInvalidValue;
		if (!args.k.upsampling && args.xr != kSrcRing) return hipErrorInvalidValue;
		// a kernel that takes its plan constants from the float block behind fir_k needs that block filled (synth_args does);
		// never with several voices: each voice's constants come from its block in LDS
		if constexpr (v2::float_arg_consts<typename S::CT, S::D, S::U, VOICES>()) {
			if (args.fir_k.f[kFirKConsts + kKfBasicIncrement] != static_cast<float>(args.k.basic_increment)) return hipErrorInvalidValue;
		}
		const size_t lds = S::lds_bytes(args.xr);
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
				static_cast<int>(lds));
		if (e != hipSuccess) return e;
		const unsigned groups = static_cast<unsigned>(VOICES ? work : (work + S::U - 1) / S::U);
		hipLaunchKernelGGL(fn, dim3(groups), dim3(S::kWaves * 64), lds, stream, args);
		return hipGetLastError();
	}
}

// What a translation unit calls, once per variant it holds: the variant's preconditions on the arguments, then one pass over
// the shapes (a stream's launch, args.stream, takes the same shapes: the ring is the stream's, args.xr).
template <int FLAGS>
static hipError_t launch_v2_variant(const SynthArgs& args, size_t work, int precision, int rows, hipStream_t stream)
{
	constexpr bool VOICES = (FLAGS & v2::kVoicesFlag) != 0, TARGETS = (FLAGS & v2::kTargetsFlag) != 0;
	if (VOICES ? !args.row_map || !args.group_voice : args.row_map != nullptr) return hipErrorInvalidValue;
	if (TARGETS && (!args.tg_offsets || !args.tg_steps || !args.tg_values || !args.frame_counts)) return hipErrorInvalidValue;
	if (TARGETS && (VOICES ? !args.tg_voice_N || !args.tg_voice_invN : args.tg_N < 1)) return hipErrorInvalidValue;
	return with_shape(precision, rows, args.k.section_delay, args.k.layout, hipErrorInvalidValue,
			[&](auto s) { return launch_v2<decltype(s), FLAGS>(args, work, stream); });
}
