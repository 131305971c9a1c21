// Reference model 5 (VocalTractModel5<double,1>, vtm/VocalTractModel5.h) on the device.
// Included inside namespace gvtm, after vtm_kernel_v2.inc (whose wave-wide DPP helpers, Extent and voice_row it shares),
// by eight translation units: vtm_kernels.hip instantiates the single-voice kernels, vtm_kernels_m5v.hip the voice variant
// (kVoices5Flag), vtm_kernels_m5f.hip the float class, VocalTractModel5<float,1> (kFloat5Flag), vtm_kernels_m5fv.hip
// the voice variant of the float class (both flags), vtm_kernels_m5t.hip and vtm_kernels_m5ft.hip the targets variant
// (kTargets5Flag) of the double and of the float class, vtm_kernels_m5tv.hip and vtm_kernels_m5ftv.hip that variant under
// several voices (kTargets5Flag with kVoices5Flag), each in a code object of its own.  Besides the kernel, the file
// defines what they launch it with: the description of its shapes (m5_shape,
// kM5Ring), before the kernel, and the LDS bytes and the launch of a shape (m5_lds_bytes, launch_synth5_shape), at the end.
//
// Same organisation as generation 2: a workgroup owns U utterances (1 or 2; the tube has 30 + 21 = 51 sections, one
// per lane of a wavefront, so every utterance has a tube wavefront of its own, while the scan, filter and interpolation
// wavefronts and the helper passes serve all of them: utterance u on lane u / lanes 2u, 2u+1 / lanes 16u..16u+15, and
// U * C <= 64 items per per-step pass), wavefronts have fixed roles, time is cut into chunks of C internal steps,
// every stage works on a different chunk in the same tick, one workgroup barrier per tick, every LDS
// buffer has as many slots as its readers lag.  Only true recurrences run in the serial wavefronts; whatever
// is a pure function of one step (or of a step and its predecessors' INPUTS) is a helper pass, one lane per step:
//
//   T   the waveguide: flow junctions, the reflected flow of the pole-zero radiation impedance at the two open ends
//       (wavefront 3: with 4 + 3 wavefronts it has a SIMD to itself)
//   S   scalar scans: Rosenberg phase t / t2, noise generator, the two noise low-passes (wavefront 1)
//   F   the recursive halves of the glottal low-pass, of the frication band-pass and of the transmitted flow (wavefront 2)
//   I   parameter interpolation, one lane per parameter (wavefront 0)
//   H   NH helpers sharing a list of parallel passes (one lane per step / per output sample) (wavefronts 4..)
//
//   tick c     I    pitch, glotVol, aspVol of chunk c (fric* lanes: chunk c-3, radii and velum: chunk c-6)  -> prm
//   tick c+1   H    A1a(c) pitch -> dt, glotVol -> amplitude and t2 target, aspVol -> amplitude          -> rd, rm
//   tick c+2   S    S(c)   t, t2, glottal noise, frication noise                                          -> rst, rn
//   tick c+3   H    B(c)   Rosenberg pulse value v from (t, t2); u = b0 (v + v[-1])                       -> val, u
//   tick c+4   F    F(c)   glottal low-pass recursion: pulse = u - a1 pulse[-1]                           -> pl
//              H    A1b(c) fricVol/Pos -> amplitude, split, first lane; fricCF/BW -> band-pass design     -> rfr, rb0, ra12
//   tick c+5   H    M(c)   source mix, tube input, glottal loss, band-pass input x; ub = b0 (x - x[-2])    -> mg, inp, fnm, ub
//   tick c+6   F    Fb(c)  band-pass recursion: y = ub - a1 y[-1] - a2 y[-2]                               -> bp
//   tick c+7   H    N(c)   glottal loss, tube input and the frication shares into the tube record         -> ru
//              H    A2(c)  radii, velum -> junction coefficients, mouth impedance                         -> ru, rmo
//   tick c+8   T    tube(c); of the radiation impedance only the reflected flow is in its loop           -> ox (flow INTO mouth, nose)
//   tick c+9   H    Y(c)   feed-forward half of the transmitted flow: cT2 in, cT3 in[-1]                  -> yv
//   tick c+10  F    Fo(c)  its recursion, mouth and nose side by side in two lanes                        -> oo
//   tick c+11  H    X(c)   mouth + nose (or the glottal signal when bypassed)                             -> x ring
//   tick c+12  H    P6(c)  sample-rate conversion, one lane per output sample                             -> y ring (float)
//   tick c+13  H    P7(c)  difference filter * output rate (VocalTractModel5.h:507-513)                    -> HBM, peak

// The kernel's four shapes, two per class, by (class, index); synth_launch_shape picks the index.
// The double class.  Index 0, one utterance per workgroup: chunk of 60 steps (one 64-lane pass per per-step stage), three
// helper wavefronts.  Index 1, two utterances per workgroup (batches beyond one workgroup per compute unit): two tube
// wavefronts, chunk of 24 steps (2 x 24 items per per-step pass; what LDS holds with two 62-entry tube records per step),
// five helpers.  Wavefronts: I, S and F, a tube wavefront per utterance, the helpers.
// The float class (VocalTractModel5<float,1>, kFloat5Flag below) has one utterance per workgroup in both, measured
// against each other in DESIGN.md 4b (profiles/r08_bench_model5_float.json).  Index 0, chunk 60 with three helpers, is
// the double shape with every record halved (84 992 B of LDS): one workgroup per compute unit, the longest chunk.
// Index 1, chunk 56 with three helpers, is the longest chunk whose workgroup stays at or below 80 KB (80 800 B), so
// that two workgroups share a compute unit.
struct M5Shape { int rows, chunk, helpers, waves, groups_per_cu; }; // groups_per_cu: workgroups a compute unit holds at once
constexpr int m5_waves(int rows, int helpers) { return 3 + rows + helpers; }
constexpr M5Shape m5_shape(bool float_class, int index)
{
	if (float_class) return index == 1 ? M5Shape{1, 56, 3, m5_waves(1, 3), 2} : M5Shape{1, 60, 3, m5_waves(1, 3), 1};
	return index == 1 ? M5Shape{2, 24, 5, m5_waves(2, 5), 1} : M5Shape{1, 60, 3, m5_waves(1, 3), 1};
}
// The targets variant (kTargets5Flag below) carries one more LDS record, f0 from pass A1a to pass X: eleven slots of a chunk.
// Its shapes, by the same (class, index), are the four above wherever the record fits the budget the shape was chosen by:
// the double class's one-utterance shape (158 928 B) has 4 912 B left of a workgroup's 160 KB where the record takes 5 280 B,
// so its chunk is the next multiple of four, 56 (156 016 B with the record); the two-utterance shape keeps 24 (152 560 B).
// The float class's index 0 keeps 60 (one workgroup per compute unit: 87 632 B); index 1, which two workgroups per compute
// unit define, has 1 120 B left of 80 KB with a chunk of 56 where the record takes 2 464 B, and takes the next multiple of
// four, 52 (78 896 B).
constexpr M5Shape m5_targets_shape(bool float_class, int index)
{
	if (float_class) return index == 1 ? M5Shape{1, 52, 3, m5_waves(1, 3), 2} : M5Shape{1, 60, 3, m5_waves(1, 3), 1};
	return index == 1 ? M5Shape{2, 24, 5, m5_waves(2, 5), 1} : M5Shape{1, 56, 3, m5_waves(1, 3), 1};
}
constexpr M5Shape m5_shape_of(bool float_class, int index, bool targets) { return targets ? m5_targets_shape(float_class, index) : m5_shape(float_class, index); }
constexpr int kM5Ring = kSrcRing; // the reference's BUFFER_SIZE: see the flush-overrun epilogue

namespace m5 {

namespace {

using v2::Extent;

// Per-step tube record.  Everything the tube wavefront reads in a step sits in ONE record of fixed size, the
// values that never change replicated into it, so that every per-lane read cursor advances by the same stride
// and the unrolled steps use immediate offsets:
//   [0..2] mouth cR1 (= cT1), cR2, cR3   [5..11] J1..J7   [12] NJ1   [13] +velum left/right   [14] -velum
//   left/right   [15] -velum upper   [16..18] nose cR1..cR3   [21] 0   [22..26] NJ2..NJ6   [28] -glottal loss
//   [30..61] what is ADDED to the new top of sections S1..S32: [30] the tube input, elsewhere 0 except the two
//   neighbouring sections the frication noise enters (:716-726)
constexpr int kRu = 62;
constexpr int kRkMouth = 0, kRkJ = 5, kRkNk = 12, kRkVl = 13, kRkNVl = 14, kRkNVu = 15, kRuNose = 16, kRuZero = 21, kRuNasal = 22,
              kRuLoss = 28, kRuAdd = 30, kAddLanes = 32, kAddNone = 30; // kAddNone: a section that never gets frication
constexpr int kRfr = 4; // A1b record: frication amplitude, left share, right share, first lane
constexpr int kMouth = 29, kNose = 50, kNasalFirst = 30, kThreeLeft = 11, kThreeRight = 12;
constexpr int kYr = 512; // ring of converted samples waiting for the difference filter
constexpr int kF0Slots = 11; // the targets variant's f0 record: written for chunk t - 1 in the tick that reads chunk t - 11

template <int C, int XR, int U = 1, typename R = double, bool TARGETS = false>
struct Offsets {
	size_t rf0 = 0; // (the targets variant's record alone, behind every other: no other offset moves)
	size_t kc, k5, ext, kb, src, prm, rd, rm, rst, rn, val, u, pl, rfr, rb0, ra12, inp, fnm, ub, bp, mg, ru, side, ox, rmo, yv, oo, carry, x, y, peak, ticket, diag, dump, total;
	__host__ __device__ constexpr Offsets()
		: kc(0), k5(0), ext(0), kb(0), src(0), prm(0), rd(0), rm(0), rst(0), rn(0), val(0), u(0), pl(0), rfr(0), rb0(0), ra12(0), inp(0), fnm(0),
		  ub(0), bp(0), mg(0), ru(0), side(0), ox(0), rmo(0), yv(0), oo(0), carry(0), x(0), y(0), peak(0), ticket(0), diag(0), dump(0), total(0)
	{
		size_t off = 0;
		auto take = [&](size_t bytes) {
			const size_t at = off;
			off += (bytes + 15) & ~size_t(15);
			return at;
		};
		constexpr size_t D = sizeof(R);
		kc = take(sizeof(DeviceConstants));
		k5 = take(sizeof(Model5Constants));
		ext = take(sizeof(Extent) * U);
		kb = take(sizeof(unsigned long long) * 4 * 2 * U); // output sample range of a chunk, (c & 3)
		src = take(sizeof(R) * (kSrcFilterLength + 1)); // h only, delta formed on the fly (26 KB for the tube records)
		prm = take(U * (sizeof(float) * 2 * C * 16));
		rd = take(U * (D * 2 * (C + 4) * 2));   // {dt, t2 target}                    A1a -> S      (c & 1)
		rm = take(U * (D * 5 * C * 2));         // {glottal, aspiration amplitude}    A1a -> M      (c % 5)
		rst = take(U * (D * 2 * C * 2));        // {t, t2}                            S -> B        (c & 1)
		rn = take(U * (D * 4 * C * 2));         // {glottal noise, frication noise}   S -> M        (c & 3)
		val = take(U * (D * 2 * C));            // pulse value                        B -> B        (c & 1)
		u = take(U * (D * 2 * (C + 4)));        // b0 (v + v[-1])                     B -> F        (c & 1)
		pl = take(U * (D * 2 * C));             // low-passed pulse                   F -> M        (c & 1)
		rfr = take(U * (D * 4 * C * kRfr));     //                                    A1b -> N      (c & 3)
		rb0 = take(U * (D * 3 * C));            // band-pass b0                       A1b -> M      (c % 3)
		ra12 = take(U * (D * 3 * (C + 4) * 2)); // band-pass {a1, a2}                 A1b -> Fb     (c % 3)
		inp = take(U * (D * 7 * C));            // tube input (bypass)                M -> X        (c % 7)
		fnm = take(U * (D * 2 * C));            // band-pass input                    M -> M        (c & 1)
		ub = take(U * (D * 2 * (C + 4)));       // b0 (x - x[-2])                     M -> Fb       (c & 1)
		bp = take(U * (D * 2 * C));             // band-pass output                   Fb -> N       (c & 1)
		mg = take(U * (D * 3 * C * 2));         // {-glottal loss, tube input}        M -> N        (c % 3)
		ru = take(U * (D * 2 * (C + 2) * kRu)); // tube record                        A2, N -> T    (c & 1)
		side = take(U * (sizeof(int) * 2 * C)); // first frication section a record slot holds (c & 1)
		ox = take(U * (D * 2 * C * 2));         // flow into {mouth, nose}            T -> Y        (c & 1)
		rmo = take(U * (D * 4 * C * 3));        // mouth {cT1, cT2, cT3}              A2 -> Y, Fo   (c & 3)
		yv = take(U * (D * 2 * (C + 2) * 4));   // {cT2 in, cT3 in[-1]} mouth, nose   Y -> Fo       (c & 1)
		oo = take(U * (D * 2 * C * 2));         // transmitted flow {mouth, nose}     Fo -> X       (c & 1)
		carry = take(U * (D * 2 * 2));          // a chunk's last inputs              Y -> Y        (c & 1)
		x = take(D * XR * U);
		y = take(sizeof(float) * kYr * U);
		peak = take(sizeof(unsigned) * 4);
		ticket = take(sizeof(unsigned) * 4);
		diag = take(sizeof(unsigned long long) * 10);
		dump = take(D * 64 * 2);
		if (TARGETS) rf0 = take(U * (D * kF0Slots * C)); // f0                               A1a -> X      (c % 11)
		total = off;
	}
};

} // namespace

// Several voices in one launch (gvtm_synthesize_voices_device on a gvtm_plan_create_model5_voices or
// gvtm_plan_create_model5_float_voices plan): the kernel's last
// template argument carries, besides the utterances per workgroup in bits 0-1, the flag kVoices5Flag (default off; one
// utterance per workgroup only).  With it, workgroup g synthesizes utterance a.row_map[g] of voice a.group_voice[g] (-1: a
// group past the last voice's, which exits at once) from that voice's constants a.kconst[voice] and a.k5const[voice].
// Everything downstream reads the staged copies; only the utterance's rows in HBM (extent, frames, samples, count, peak,
// stream state) follow the row map.  As in vtm_kernel_v2.inc (kVoicesFlag), each voice-dependent expression is a conditional on the
// constant VOICES, so the single-voice kernels compile to the code they had before the flag existed.
constexpr int kVoices5Flag = 4;
// VocalTractModel5<float,1> (gvtm_plan_create_model5_float and _float_voices; instantiated by vtm_kernels_m5f.hip and, with
// kVoices5Flag, vtm_kernels_m5fv.hip alone, which compile with FMA contraction off): the flag kFloat5Flag in the same
// argument makes R, the type of every LDS record, every recurrence
// and the tube, float instead of double.  The constants arrive as floats widened in the double fields of DeviceConstants /
// Model5Constants and are narrowed where they are used (R(k5.x): exact); the resampler's table is the float design's; a
// stream's state keeps its double slots (Stream5Layout), a float stored widened being exact; the noise generator's seed
// stays double (NoiseSource.h:41-54).  With R = double every R(...) below is the identity, so the double kernels are
// the code they were.
constexpr int kFloat5Flag = 8;
// The model as the editor's interactive window runs it (gvtm_synthesize_targets_model5_device; instantiated by
// vtm_kernels_m5t.hip and, with kFloat5Flag, vtm_kernels_m5ft.hip alone): VocalTractModel5<T,1>(config, interactive = true)
// fed parameter targets.  The flag kTargets5Flag in the same argument changes two things.  The interpolation wavefront walks
// the moving averages of the utterance's sixteen target lists (vtm_targets.hpp) instead of interpolating frames: a.frame_counts
// holds steps, there are no frames and no control_steps.  And what enters the resampler is divided by the step's
// fundamental frequency (VocalTractModel5.h:579): pass A1a keeps the f0 it forms for dt in the record rf0, which pass X
// reads ten ticks later.  One voice, or with kVoices5Flag several (see the interpolation wavefront's
// setup).  A stream's launches (gvtm_stream_push_targets_model5, several voices: _model5_voices) walk absolute steps from the
// utterance's step_base on: behind step 0 the walk resumes on the 16 sums the previous launch left in the stream state
// (targets_resume, Stream5Layout::sums; the points are the stream's log), and the epilogue stores them back.  The record rf0
// carries nothing from launch to launch: chunk c's slot, c % 11, is written by A1a at tick c + 1 and read by X at tick
// c + 11 of the same launch -- the tick loop drains every chunk through X (max_chunks + 14 ticks) -- and c restarts at 0 with
// every launch.  Every difference is a conditional on the constant TARGETS.
constexpr int kTargets5Flag = 16;
__device__ __forceinline__ double sin_m5(double t) { return sin(t); }
__device__ __forceinline__ float sin_m5(float t) { return vmath::sinf_glibc(t); } // std::sin(float), RosenbergBGlottalSource.h:139

// wavefronts per SIMD a shape is compiled for: a shape of which a compute unit holds two workgroups (the float class's
// 80 KB shape) must leave room for the second (7 + 7 wavefronts: four on a SIMD, 128 registers each); every other shape
// gets what its workgroup size implies (a request below that is no request)
constexpr int m5_waves_per_simd(int chunk, int u_flags)
{
	for (int index = 0; index < 2; ++index) {
		const M5Shape s = m5_shape_of((u_flags & kFloat5Flag) != 0, index, (u_flags & kTargets5Flag) != 0);
		if (s.chunk == chunk && s.groups_per_cu > 1) return (s.groups_per_cu * s.waves + 3) / 4;
	}
	return 1;
}

template <int C, int NH, int XR, int U_FLAGS>
__global__ __launch_bounds__(m5_waves(U_FLAGS & 3, NH) * 64, m5_waves_per_simd(C, U_FLAGS)) void vtm5_synth_kernel(const SynthArgs a)
{
	constexpr int U = U_FLAGS & 3;
	constexpr bool VOICES = (U_FLAGS & kVoices5Flag) != 0;
	constexpr bool FLOAT = (U_FLAGS & kFloat5Flag) != 0;
	constexpr bool TARGETS = (U_FLAGS & kTargets5Flag) != 0;
	using R = std::conditional_t<FLOAT, float, double>;
	using R2 = typename Pair<R>::type;
	static_assert(!FLOAT || U == 1, "the float class has the one-utterance shape only");
	static_assert(!VOICES || U == 1, "the voice variant has the one-utterance shape only");
	int voice = 0;
	if constexpr (VOICES) {
		voice = a.group_voice[blockIdx.x];
		if (voice < 0) return; // (uniform across the workgroup, before any barrier)
	}
	static_assert(U == 1 || U == 2, "one or two utterances per workgroup");
	static_assert(C % 4 == 0 && U * C <= 64, "one helper pass per per-step stage, serial stages in blocks of four");
	static_assert((XR & (XR - 1)) == 0 && XR >= 2 * C + 4 * kMaxPad, "ring must hold 2 chunks + history + flush");
	constexpr int kThreads = (3 + U + NH) * 64;
	// elements one utterance owns in each LDS region (Offsets reserves U times as much)
	constexpr int kN_prm = 2 * C * 16, kN_rd = 2 * (C + 4) * 2, kN_rm = 5 * C * 2, kN_rst = 2 * C * 2, kN_rn = 4 * C * 2, kN_val = 2 * C,
	              kN_u = 2 * (C + 4), kN_pl = 2 * C, kN_rfr = 4 * C * kRfr, kN_rb0 = 3 * C, kN_ra12 = 3 * (C + 4) * 2, kN_inp = 7 * C,
	              kN_fnm = 2 * C, kN_ub = 2 * (C + 4), kN_bp = 2 * C, kN_mg = 3 * C * 2, kN_ru = 2 * (C + 2) * kRu, kN_side = 2 * C,
	              kN_ox = 2 * C * 2, kN_rmo = 4 * C * 3, kN_yv = 2 * (C + 2) * 4, kN_oo = 2 * C * 2, kN_carry = 4;

	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	constexpr Offsets<C, XR, U, R, TARGETS> so;
	[[maybe_unused]] constexpr int kN_rf0 = kF0Slots * C;
	[[maybe_unused]] R* const s_rf0 = reinterpret_cast<R*>(smem_raw + so.rf0); // (the targets variant's alone)
	DeviceConstants* const s_kc = reinterpret_cast<DeviceConstants*>(smem_raw + so.kc);
	Model5Constants* const s_k5 = reinterpret_cast<Model5Constants*>(smem_raw + so.k5);
	Extent* const s_ext = reinterpret_cast<Extent*>(smem_raw + so.ext);
	unsigned long long* const s_kb = reinterpret_cast<unsigned long long*>(smem_raw + so.kb);
	R* const s_src = reinterpret_cast<R*>(smem_raw + so.src);
	int* const s_side = reinterpret_cast<int*>(smem_raw + so.side);
	float* const s_prm = reinterpret_cast<float*>(smem_raw + so.prm);
	auto dptr = [&](size_t off) { return reinterpret_cast<R*>(smem_raw + off); };
	R* const s_rd = dptr(so.rd);
	R* const s_rm = dptr(so.rm);
	R* const s_rst = dptr(so.rst);
	R* const s_rn = dptr(so.rn);
	R* const s_val = dptr(so.val);
	R* const s_u = dptr(so.u);
	R* const s_pl = dptr(so.pl);
	R* const s_rfr = dptr(so.rfr);
	R* const s_rb0 = dptr(so.rb0);
	R* const s_ra12 = dptr(so.ra12);
	R* const s_inp = dptr(so.inp);
	R* const s_fnm = dptr(so.fnm);
	R* const s_ub = dptr(so.ub);
	R* const s_bp = dptr(so.bp);
	R* const s_mg = dptr(so.mg);
	R* const s_ru = dptr(so.ru);
	R* const s_ox = dptr(so.ox);
	R* const s_rmo = dptr(so.rmo);
	R* const s_yv = dptr(so.yv);
	R* const s_oo = dptr(so.oo);
	R* const s_carry = dptr(so.carry);
	R* const s_x = dptr(so.x);
	R* const s_x_all = s_x;
	float* const s_y = reinterpret_cast<float*>(smem_raw + so.y);
	unsigned* const s_peak = reinterpret_cast<unsigned*>(smem_raw + so.peak);
	unsigned* const s_ticket = reinterpret_cast<unsigned*>(smem_raw + so.ticket);
	R* const s_dump = dptr(so.dump);
	unsigned long long* const s_diag = reinterpret_cast<unsigned long long*>(smem_raw + so.diag);

	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int wave = tid >> 6;
	// Wavefront w of a workgroup lands on SIMD w mod 4.  One utterance: with 4 + 3 wavefronts the fourth has a SIMD to
	// itself, which goes to the tube (the longest chain); the interpolation wavefront shares SIMD 0 with a helper.  Two
	// utterances: the two tube wavefronts are wavefronts 0 and 1 (different SIMDs), then scan, filters, interpolation.
	constexpr int kFirstHelper = 3 + U;
	constexpr bool kBoundsRecurrence = sizeof(R) == 8; // the resampler's output ranges by running remainder (stage_bounds)
	int role;           // 0 T, 1 S, 2 F, 3 I, 4 helpers
	int tube_u = 0;     // utterance of a tube wavefront
	if constexpr (U == 1) {
		role = wave == 3 ? 0 : (wave == 0 ? 3 : (wave < 4 ? wave : 4));
	} else {
		role = wave < U ? 0 : (wave < kFirstHelper ? wave - U + 1 : 4);
		tube_u = wave < U ? wave : 0;
	}
	const size_t group = blockIdx.x;
	// GVTM_M5_UTT(u, single-voice expression): the utterance of row u (see kVoices5Flag; a voice's group is never empty)
#define GVTM_M5_UTT(u, ...) (VOICES ? v2::voice_row(a, group * U + (u)) : __VA_ARGS__)

	// ---- constants, extent and the resampler table into LDS; clear the rings
	{
		const int* src = reinterpret_cast<const int*>(VOICES ? a.kconst + voice : a.kconst);
		int* dst = reinterpret_cast<int*>(s_kc);
		for (int i = tid; i < static_cast<int>(sizeof(DeviceConstants) / sizeof(int)); i += kThreads) dst[i] = src[i];
		const int* src5 = reinterpret_cast<const int*>(VOICES ? a.k5const + voice : a.k5const);
		int* dst5 = reinterpret_cast<int*>(s_k5);
		for (int i = tid; i < static_cast<int>(sizeof(Model5Constants) / sizeof(int)); i += kThreads) dst5[i] = src5[i];
	}
	for (int i = tid; i <= kSrcFilterLength; i += kThreads) {
		s_src[i] = i < kSrcFilterLength ? static_cast<const R*>(a.src_h)[i] : R(0.0); // deltaH_[last] = 0 - h_[last] (SampleRateConverter.h:254)
	}
	for (int i = tid; i < U * kN_ru; i += kThreads) s_ru[i] = R(0.0);
	for (int i = tid; i < U * kN_side; i += kThreads) s_side[i] = kAddNone;
	for (int i = tid; i < U * XR; i += kThreads) s_x[i] = R(0.0);
	for (int i = tid; i < U * kYr; i += kThreads) s_y[i] = 0.0f;
	__syncthreads();
	const DeviceConstants& k = *s_kc;
	const Model5Constants& k5 = *s_k5;
	// gvtm_stream_*: a launch continues utterances from the state an earlier launch left in device memory (a.stream,
	// layout: Stream5Layout in vtm_kernels.hpp) and leaves its own behind.  A push synthesizes whole frames, keeps the
	// converter's flush for later and finds the frame AFTER its last one in the buffer; finish (and the one-shot entry) flushes.
	// (the voice variant streams too: every stream-state address follows the row map, GVTM_M5_UTT)
	const bool kPush = a.stream_mode == kStreamPush;
	const bool kFinal = !kPush;
	const bool streaming = a.stream != nullptr;
	if (tid < U) {
		Extent e{0, 0, 0, 0, 0ull, 0ull};
		const size_t ug = GVTM_M5_UTT(tid, group * U + tid);
		unsigned peak0 = 0u;
		if (ug < a.batch) {
			// a stream's push carries one more row than it synthesizes: the next frame, which the last one interpolates towards
			// (not from targets: no step waits for a successor)
			const size_t rows_avail = a.max_frames - (kPush && !TARGETS ? 1 : 0);
			const int f = a.frame_counts ? a.frame_counts[ug] : static_cast<int>(rows_avail);
			e.frames = f > 0 ? (static_cast<size_t>(f) < rows_avail ? f : static_cast<int>(rows_avail)) : 0;
			if constexpr (TARGETS) e.steps = static_cast<uint32_t>(e.frames); // (a.frame_counts holds steps; a refused utterance's: 0)
			else e.steps = static_cast<uint32_t>(e.frames) * k.control_steps;
			e.nchunks = e.steps == 0 ? 1 : static_cast<int>((e.steps + C - 1) / C);
			e.last_frame = e.frames - 1 + (kPush ? 1 : 0);
			if (streaming) {
				const StreamHeader* h = reinterpret_cast<const StreamHeader*>(a.stream + ug * a.stream_stride);
				e.step_base = h->step_base;
				e.k_first = ((e.step_base << 16) + k.time_inc - 1) / k.time_inc;
				peak0 = h->peak_bits;
			}
		}
		s_ext[tid] = e; // (a slot beyond the batch: nchunks 0, nothing runs for it)
		s_peak[tid] = peak0;
	}
	if (tid == 0) s_ticket[0] = s_ticket[1] = 0u;
	if constexpr (kBoundsRecurrence) {
		if (tid == 0) {
			const SrcBoundsStep bstep = src_bounds_step(k.time_inc, C); // (the two spare words behind the counters: stage_bounds)
			s_ticket[2] = bstep.dq;
			s_ticket[3] = bstep.dr;
		}
	}
	if (tid < 10) s_diag[tid] = 0ull;
	__syncthreads();

	if (streaming) {
		// the two rings, and what the feed-forward halves of the filters need from the step before this launch's first one
		for (int u = 0; u < U; ++u) {
			if (GVTM_M5_UTT(u, group * U + u) >= a.batch) break;
			const unsigned char* sb = a.stream + GVTM_M5_UTT(u, (group * U + u)) * a.stream_stride;
			const double* ring = reinterpret_cast<const double*>(sb + Stream5Layout::ring());
			for (int i = tid; i < XR; i += kThreads) s_x[u * XR + i] = static_cast<R>(ring[i]);
			const float* yr = reinterpret_cast<const float*>(sb + Stream5Layout::yring());
			for (int i = tid; i < kYr; i += kThreads) s_y[u * kYr + i] = yr[i];
			if (tid == 0) {
				const double* sc = reinterpret_cast<const double*>(sb + Stream5Layout::scalars());
				// (chunk 0 looks for its predecessor's last values in slot 1, where chunk -1 would have left them)
				s_val[u * kN_val + C + C - 1] = static_cast<R>(sc[kS5ValLast]);
				s_fnm[u * kN_fnm + C + C - 2] = static_cast<R>(sc[kS5FnmLast]);
				s_fnm[u * kN_fnm + C + C - 1] = static_cast<R>(sc[kS5FnmLast + 1]);
				s_carry[u * kN_carry + 2] = static_cast<R>(sc[kS5Carry]);
				s_carry[u * kN_carry + 3] = static_cast<R>(sc[kS5Carry + 1]);
			}
		}
		__syncthreads();
	}
	int max_chunks = 0;
#pragma unroll
	for (int u = 0; u < U; ++u) max_chunks = s_ext[u].nchunks > max_chunks ? s_ext[u].nchunks : max_chunks;
	// steps of utterance u inside chunk c: -1 = the chunk does not exist for it
	auto valid_in = [&](int u, int c) -> int {
		const Extent e = s_ext[u];
		if (c < 0 || c >= e.nchunks) return -1;
		const uint32_t left = e.steps - static_cast<uint32_t>(c) * C;
		return left < static_cast<uint32_t>(C) ? static_cast<int>(left) : C;
	};
	// the longest run any utterance of the workgroup has in chunk c (the shared serial wavefronts run that long; an
	// utterance that has ended runs on over stale inputs, its results are never consumed)
	auto valid_any = [&](int c) -> int {
		int v = -1;
#pragma unroll
		for (int u = 0; u < U; ++u) { const int w = valid_in(u, c); v = w > v ? w : v; }
		return v;
	};
	// a helper pass's item: lane = u * C + s
	const int item_u = lane / C, item_s = lane - item_u * C;

	// -------------------------------------------------------------------------------------
	// helper passes (one lane per step unless said otherwise)

	// A1a: pitch, glottal volume, aspiration volume (execSynthesisStep :528-531, RosenbergBGlottalSource::setup)
	auto stage_a1a = [&](int c) {
		const int u = item_u, s = item_s;
		if (u >= U || s >= valid_in(u, c)) return;
		const float* pv = s_prm + u * kN_prm + (static_cast<size_t>(c & 1) * C + s) * 16;
		const R pitch = pv[0], gv = pv[1], av = pv[2];
		const R f0 = frequency_dev(pitch);
		const R ga = amplitude_60db_dev(gv);
		R* rd = s_rd + u * kN_rd + (static_cast<size_t>(c & 1) * (C + 4) + s) * 2;
		rd[0] = f0 / R(k5.sample_rate);
		if constexpr (TARGETS) s_rf0[u * kN_rf0 + (c % kF0Slots) * C + s] = f0; // what pass X divides the step's signal by
		// the amplitude-dependent end of the falling phase: a pure function of the amplitude (setup() skips the
		// assignment only when it would store the same value)
		rd[1] = (R(k5.rb_tn_min) == R(k5.rb_tn_max)) ? R(k5.rb_t1) + R(k5.rb_tn_max)
		                                       : R(k5.rb_t1) + R(k5.rb_tn_max) - ga * (R(k5.rb_tn_max) - R(k5.rb_tn_min));
		R* rm = s_rm + u * kN_rm + (static_cast<size_t>(c % 5) * C + s) * 2;
		rm[0] = ga;
		rm[1] = amplitude_60db_dev(av);
	};

	// A1b: the frication parameters (:716-721; BandpassFilter::update)
	auto stage_a1b = [&](int c) {
		const int u = item_u, s = item_s;
		if (u >= U || s >= valid_in(u, c)) return;
		const float* pv = s_prm + u * kN_prm + (static_cast<size_t>(c & 1) * C + s) * 16;
		const R fvol = pv[3], fpos = pv[4], fcf = pv[5], fbw = pv[6];
		R* r = s_rfr + u * kN_rfr + (static_cast<size_t>(c & 3) * C + s) * kRfr;
		const R offset = (27 - 5) * (fpos / R(7.0));
		// inside the tube: the section S6 + (int) offset is one of S1..S30, the reference's own arithmetic.  Outside, the
		// reference indexes its array out of bounds; the product injects nothing (include/gama_vtm.h): the record names
		// the section kAddNone, which pass N drops.  Decided on the floating offset, so that no cast of a value beyond
		// the range of int and no wrapped sum is relied upon.
		const bool inside = offset > R(-6.0) && offset < R(25.0);
		const int oi = inside ? static_cast<int>(offset) : kAddNone - 5;
		const R right = offset - oi;
		r[0] = amplitude_60db_dev(fvol);
		r[1] = R(1.0) - right;
		r[2] = (5 + oi < 27) ? right : R(0.0); // the right neighbour only gets its share below S28 (:723-725)
		r[3] = static_cast<R>(5 + oi);
		const R pi = R(3.14159265358979323846);
		const R tan_v = tan_dev(pi * fbw * R(k.bp_T));
		const R cos_v = cos_dev(R(2.0) * pi * fcf * R(k.bp_T));
		const R a2 = (R(1.0) - tan_v) / (R(1.0) + tan_v);
		s_rb0[u * kN_rb0 + (c % 3) * C + s] = R(0.5) - R(0.5) * a2;
		R* a12 = s_ra12 + u * kN_ra12 + (static_cast<size_t>(c % 3) * (C + 4) + s) * 2;
		a12[0] = -(R(1.0) + a2) * cos_v;
		a12[1] = a2;
	};

	// A2: radii and velum -> calculateTubeCoefficients (VocalTractModel5.h:614-634)
	auto stage_a2 = [&](int c) {
		const int u = item_u, s = item_s;
		if (u >= U || s >= valid_in(u, c)) return;
		const float* cur = s_prm + u * kN_prm + (static_cast<size_t>(c & 1) * C + s) * 16 + 7;
		R r2[8];
		R r8 = R(0.0);
#pragma unroll
		for (int q = 0; q < 8; ++q) {
			R r = static_cast<R>(cur[q]) * R(k.radius_coef[q]);
			r = r > R(0.01) ? r : R(0.01); // GS_VTM5_MIN_RADIUS
			r2[q] = r * r;
			r8 = r;
		}
		const R velum = cur[8];
		const R v2 = velum * velum;
		R* rk = s_ru + u * kN_ru + (static_cast<size_t>(c & 1) * (C + 2) + s) * kRu;
#pragma unroll
		for (int q = 0; q < 7; ++q) rk[kRkJ + q] = (r2[q] - r2[q + 1]) / (r2[q] + r2[q + 1]);
		rk[kRkNk] = (v2 - R(k5.nasal_r1_sq)) / (v2 + R(k5.nasal_r1_sq));
		// Junction3::configure(r4, r4, velum): left and right coefficients coincide.  The lanes that take the
		// junction's outputs through their LEFT link read the negated value (their formula subtracts).
		const R cc = R(1.0) / (r2[3] + r2[3] + v2);
		const R vl = cc * ((r2[3] - r2[3]) - v2);
		const R vu = cc * ((v2 - r2[3]) - r2[3]);
		rk[kRkVl] = vl;
		rk[kRkNVl] = -vl;
		rk[kRkNVu] = -vu;
		// the values that never change, replicated (see kRu)
#pragma unroll
		for (int q = 0; q < 5; ++q) rk[kRuNasal + q] = R(k5.nasal_k[q + 1]);
		// the tube only needs the reflection side of an impedance: cR1 (= cT1), cR2, cR3 (k5.*_c: cT1, cT2, cT3, cR1, cR2, cR3)
		rk[kRuNose + 0] = R(k5.nose_c[3]);
		rk[kRuNose + 1] = R(k5.nose_c[4]);
		rk[kRuNose + 2] = R(k5.nose_c[5]);
		rk[kRuZero] = R(0.0);
		R* rmo = s_rmo + u * kN_rmo + (static_cast<size_t>(c & 3) * C + s) * 3; // the transmission side, for Y and Fo
		if (k5.constant_mouth) {
			rk[kRkMouth + 0] = R(k5.mouth_c[3]);
			rk[kRkMouth + 1] = R(k5.mouth_c[4]);
			rk[kRkMouth + 2] = R(k5.mouth_c[5]);
			rmo[0] = R(k5.mouth_c[0]);
			rmo[1] = R(k5.mouth_c[1]);
			rmo[2] = R(k5.mouth_c[2]);
		}
		if (!k5.constant_mouth) {
			// PoleZeroRadiationImpedance::update (vtm/PoleZeroRadiationImpedance.h:139-177), radius in metres
			const R radius = r8 * static_cast<R>(1.0e-2f);
			const R transition = R(0.5e-2);
			const R rr = radius < transition ? transition : radius;
			const R trans_freq = R(62.3371) / rr + R(320.204);
			const R cos_wt = cos_dev(R(2.0 * 3.14159265358979323846) * trans_freq * R(k5.period));
			const R qa = R(2.0) * cos_wt;
			const R qb = -R(2.0) * (cos_wt + R(1.0));
			const R qc = cos_wt + R(1.0);
			const R delta = qb * qb - R(4.0) * qa * qc;
			R aa = (-qb - sqrt(delta)) / (R(2.0) * qa);
			const R bb = R(2.0) * aa - R(1.0);
			if (radius < transition) aa *= R(40391.2) * (radius * radius);
			const R coef = R(1.0) / (aa + R(1.0));
			const R c1 = (aa + bb) * coef;
			rk[kRkMouth + 0] = c1;                // cR1 = cT1
			rk[kRkMouth + 1] = (aa - R(1.0)) * coef; // cR2
			rk[kRkMouth + 2] = (bb - aa) * coef;  // cR3
			rmo[0] = c1;
			rmo[1] = R(2.0) * coef;                  // cT2
			rmo[2] = -R(2.0) * bb * coef;            // cT3
		}
	};

	// B: RosenbergBGlottalSource::getSample's value for the phase the scan recorded, and the feed-forward half of
	// the glottal low-pass (Butterworth1LowPassFilter::filter: y = b0 (x + x1) - a1 y1)
	auto stage_b = [&](int c) {
		const int u = item_u < U ? item_u : U - 1, s = item_s;
		const int valid = item_u < U ? valid_in(u, c) : -1;
		R value = R(0.0);
		if (s < valid) {
			const R* rs = s_rst + u * kN_rst + (static_cast<size_t>(c & 1) * C + s) * 2;
			const R t = rs[0], t2 = rs[1];
			if (k.waveform == 0) {
				if (t < R(k5.rb_t1)) {
					const R x = t / R(k5.rb_t1);
					value = (x * x) * (R(3.0) - R(2.0) * x);
				} else if (t < t2) {
					const R x = (t - R(k5.rb_t1)) / (t2 - R(k5.rb_t1));
					value = R(1.0) - x * x;
				}
			} else {
				value = sin_m5(t * R(2.0 * 3.14159265358979323846));
			}
			s_val[u * kN_val + (c & 1) * C + s] = value;
		}
		R prev = __shfl_up(value, 1);
		if (s == 0) prev = (c > 0 || streaming) ? s_val[u * kN_val + ((c - 1) & 1) * C + C - 1] : R(0.0);
		if (s < valid) s_u[u * kN_u + (c & 1) * (C + 4) + s] = R(k5.gp_b0) * (value + prev);
	};

	// M: source mix, tube input, glottal loss (VocalTractModel5.h:553-573) and the feed-forward half of the
	// frication band-pass (BandpassFilter::filter: y = b0 (x - x2) - a1 y1 - a2 y2)
	auto stage_m = [&](int c) {
		const int u = item_u < U ? item_u : U - 1, s = item_s;
		const int valid = item_u < U ? valid_in(u, c) : -1;
		R fn = R(0.0);
		if (s < valid) {
			const R pulse = s_pl[u * kN_pl + (c & 1) * C + s];
			const R* rn = s_rn + u * kN_rn + (static_cast<size_t>(c & 3) * C + s) * 2;
			const R* rm = s_rm + u * kN_rm + (static_cast<size_t>(c % 5) * C + s) * 2;
			const R gn = rn[0], ga = rm[0], asp = rm[1];
			fn = rn[1];
			const R bf = R(k.breathiness);
			const R pulsed_noise = gn * pulse;
			const R noisy_pulse = ga * (pulse * (R(1.0) - bf) + pulsed_noise * bf);
			if (k.modulation) {
				R cm = ga * R(k.crossmix_factor);
				cm = cm < R(1.0) ? cm : R(1.0);
				fn = fn * (noisy_pulse * cm + (R(1.0) - cm));
			}
			const R input = noisy_pulse + asp * fn;
			const R min_l = R(1.0) - ga * R(k5.min_loss);
			const R max_l = R(1.0) - ga * R(k5.max_loss);
			const R gloss = min_l + (max_l - min_l) * pulse;
			R* mg = s_mg + u * kN_mg + (static_cast<size_t>(c % 3) * C + s) * 2;
			mg[0] = -gloss; // S1's left link computes X - k P
			mg[1] = input;
			s_inp[u * kN_inp + (c % 7) * C + s] = input;
			s_fnm[u * kN_fnm + (c & 1) * C + s] = fn;
		}
		R x2 = __shfl_up(fn, 2);
		if (s < 2) x2 = (c > 0 || streaming) ? s_fnm[u * kN_fnm + ((c - 1) & 1) * C + C - 2 + s] : R(0.0);
		if (s < valid) s_ub[u * kN_ub + (c & 1) * (C + 4) + s] = s_rb0[u * kN_rb0 + (c % 3) * C + s] * (fn - x2);
	};

	// N: frication amplitude and its split over two neighbouring sections (:716-726)
	auto stage_n = [&](int c) {
		const int u = item_u, s = item_s;
		if (u >= U || s >= valid_in(u, c)) return;
		const R* r = s_rfr + u * kN_rfr + (static_cast<size_t>(c & 3) * C + s) * kRfr;
		const R fv = r[0] * (R(k5.frication_factor) * s_bp[u * kN_bp + (c & 1) * C + s]);
		const R* mg = s_mg + u * kN_mg + (static_cast<size_t>(c % 3) * C + s) * 2;
		R* ru = s_ru + u * kN_ru + (static_cast<size_t>(c & 1) * (C + 2) + s) * kRu;
		ru[kRuLoss] = mg[0];
		// the dense "added to the new top" lanes: clear what this record held two chunks ago, then S1 <- tube input and
		// the two frication sections, any of S1..S30 (A1b names kAddNone for a position outside the tube: nothing is
		// injected).  S1's lane holds the tube input, so its share is folded into that: bottom * loss + (input + share)
		// where the reference has (bottom * loss + input) + share (:652, :722), one rounding away (DESIGN.md 4b)
		int* side = s_side + u * kN_side + (c & 1) * C + s;
		const int old = *side;
		R* add = ru + kRuAdd;
		add[old] = R(0.0);
		add[old + 1] = R(0.0);
		const int fl = static_cast<int>(r[3]);
		const bool in_tube = static_cast<unsigned>(fl) < static_cast<unsigned>(kAddNone);
		const int at = in_tube ? fl : kAddNone;
		const R left = fv * r[1];
		add[at] = in_tube ? left : R(0.0);
		add[at + 1] = in_tube ? fv * r[2] : R(0.0);
		add[0] = fl == 0 ? mg[1] + left : mg[1];
		*side = at;
	};

	// Y: the transmitted flow of the two radiation impedances (PoleZeroRadiationImpedance::process: outT = cT1 outT1 +
	// cT2 in + cT3 in1) is not part of the tube's feedback loop: the tube records the flow INTO mouth and nose, this
	// pass forms cT2 in and cT3 in[-1], the recursion runs a tick later in the filter wavefront (Fo)
	auto stage_y = [&](int c) {
		const int u = item_u < U ? item_u : U - 1, s = item_s;
		const int valid = item_u < U ? valid_in(u, c) : -1;
		R in_m = R(0.0), in_n = R(0.0);
		if (s < valid) {
			const R* ox = s_ox + u * kN_ox + (static_cast<size_t>(c & 1) * C + s) * 2;
			in_m = ox[0];
			in_n = ox[1];
		}
		R pm = __shfl_up(in_m, 1), pn = __shfl_up(in_n, 1);
		if (s == 0) {
			pm = (c > 0 || streaming) ? s_carry[u * kN_carry + ((c - 1) & 1) * 2] : R(0.0);
			pn = (c > 0 || streaming) ? s_carry[u * kN_carry + ((c - 1) & 1) * 2 + 1] : R(0.0);
		}
		if (s < valid) {
			const R* rmo = s_rmo + u * kN_rmo + (static_cast<size_t>(c & 3) * C + s) * 3;
			R* yv = s_yv + u * kN_yv + (static_cast<size_t>(c & 1) * (C + 2) + s) * 4;
			yv[0] = rmo[1] * in_m;
			yv[1] = rmo[2] * pm;
			yv[2] = R(k5.nose_c[1]) * in_n;
			yv[3] = R(k5.nose_c[2]) * pn;
		}
		if (s == valid - 1 && item_u < U) { // (a chunk's last step: the next chunk's -- or the next launch's -- predecessor)
			s_carry[u * kN_carry + (c & 1) * 2] = in_m;
			s_carry[u * kN_carry + (c & 1) * 2 + 1] = in_n;
		}
	};

	// X: what enters the resampler (VocalTractModel5.h:566-579) -> internal-rate ring; the 2*pad flush zeros
	// follow the utterance (SampleRateConverter.h:462-471)
	auto stage_x = [&](int c) {
		{
			const int u = item_u, s = item_s;
			if (u < U && s < valid_in(u, c)) {
				const uint32_t n0 = static_cast<uint32_t>(s_ext[u].step_base) + static_cast<uint32_t>(c) * C; // ring slots go by the stream's sample number
				const R* oo = s_oo + u * kN_oo + (static_cast<size_t>(c & 1) * C + s) * 2;
				const R v = k5.bypass ? s_inp[u * kN_inp + (c % 7) * C + s] : oo[0] + oo[1];
				// (interactive_: signal / f0, one correctly rounded division in R, VocalTractModel5.h:579; the flush's zeros below
				// are the converter's own and are not divided)
				if constexpr (TARGETS) s_x[u * XR + ((n0 + s) & (XR - 1))] = v / s_rf0[u * kN_rf0 + (c % kF0Slots) * C + s];
				else s_x[u * XR + ((n0 + s) & (XR - 1))] = v;
			}
		}
		if (kFinal) {
#pragma unroll
			for (int u = 0; u < U; ++u) {
				const Extent e = s_ext[u];
				if (c == e.nchunks - 1 && valid_in(u, c) >= 0) {
					for (int i = lane; i < 2 * k.pad; i += 64) s_x[u * XR + ((static_cast<uint32_t>(e.step_base) + e.steps + i) & (XR - 1))] = R(0.0);
				}
			}
		}
	};

	// output sample range of chunk c: sample ko is produced once its read position floor(ko * inc / 2^16)
	// lies before the filled length
	// (once per chunk, by an idle lane of the interpolation wavefront, one tick before the resampler needs them.  In the
	// double class the lane carries quotient and remainder of ceil((step_base + c * C) * 2^16 / time_inc) from chunk to chunk
	// -- src_bounds_advance, csrc/vtm_design.hpp; chunk 0's quotient is k_first, one multiplication gives its remainder -- and
	// divides out only the end of the last chunk, which is no whole chunk away: 256 x 500 frames 13.847 -> 13.741 ms
	// (profiles/bounds_recurrence_ab.md).  The float class, which bench.py cannot time, keeps the two emulated 64-bit divisions
	// per chunk.)
	[[maybe_unused]] SrcBounds bnd{0ull, 0u};
	if constexpr (kBoundsRecurrence) {
		if (role == 3 && lane >= 16 * U && lane < 16 * U + U) {
			const Extent e = s_ext[lane - 16 * U];
			bnd.q = e.k_first;
			bnd.r = static_cast<unsigned>((e.step_base << 16) + k.time_inc - 1 - e.k_first * k.time_inc);
		}
	}
	auto stage_bounds = [&](int u, int c) {
		if (c < 0 || c >= max_chunks) return;
		const Extent e = s_ext[u];
		unsigned long long lo = 0, hi = 0; // (a chunk the utterance does not have: an empty range)
		if constexpr (kBoundsRecurrence) {
			const unsigned long long q0 = bnd.q;
			src_bounds_advance(bnd, SrcBoundsStep{s_ticket[2], s_ticket[3]}, k.time_inc);
			if (c < e.nchunks) {
				lo = q0;
				hi = (c == e.nchunks - 1) ? src_bounds_at(k.time_inc, e.step_base + e.steps + (kFinal ? 2ull * k.pad : 0ull)).q : bnd.q;
			}
		} else if (c < e.nchunks) {
			const uint64_t n0 = e.step_base + static_cast<uint64_t>(c) * C;
			const uint64_t filled = (c == e.nchunks - 1) ? e.step_base + e.steps + (kFinal ? 2ull * k.pad : 0ull) : n0 + C;
			lo = c == 0 ? e.k_first : ((n0 << 16) + k.time_inc - 1) / k.time_inc;
			hi = ((filled << 16) + k.time_inc - 1) / k.time_inc;
		}
		s_kb[((c & 3) * U + u) * 2] = lo;
		s_kb[((c & 3) * U + u) * 2 + 1] = hi;
	};
	auto out_range = [&](int u, int c, uint64_t& k_lo, uint64_t& k_hi) {
		k_lo = s_kb[((c & 3) * U + u) * 2];
		k_hi = s_kb[((c & 3) * U + u) * 2 + 1];
	};

	// P6: SampleRateConverter::dataEmpty (SampleRateConverter.h:295-416) evaluated per output sample
	// the converter's output sample ko from the ring as it stands
	auto src_value = [&](int u, uint64_t ko) -> float {
		const R* const s_x = s_x_all + u * XR; // (this utterance's ring)
		const uint64_t t = ko * k.time_inc;
		const int base = static_cast<int>(t >> 16) - k.pad; // ring index p holds internal sample p - pad
		const unsigned frac = static_cast<unsigned>(t & 0xFFFFu);
		R acc = R(0.0);
		// {h, deltaH} of a tap: deltaH_[i] = h_[i+1] - h_[i] as initializeFilter formed it (SampleRateConverter.h:250-254)
		auto src_tap = [&](unsigned i) {
			const R h0 = s_src[i], h1 = s_src[i + 1];
			return SrcTap<R>{h0, h1 - h0};
		};
		if (k.upsampling) {
			const unsigned l = frac >> 8, m = frac & 0xFFu;
			const R interp = static_cast<R>(m) / R(256.0);
#pragma unroll
			for (int j = 0; j < kSrcZeroCrossings; ++j) {
				const SrcTap<R> cf = src_tap(l + 256 * j);
				acc += s_x[(base - j) & (XR - 1)] * (cf.h + cf.dh * interp);
			}
			const unsigned nfrac = (~frac) & 0xFFFFu;
			const unsigned l2 = nfrac >> 8, m2 = nfrac & 0xFFu;
			const R interp2 = static_cast<R>(m2) / R(256.0);
#pragma unroll
			for (int j = 0; j < kSrcZeroCrossings; ++j) {
				const SrcTap<R> cf = src_tap(l2 + 256 * j);
				acc += s_x[(base + 1 + j) & (XR - 1)] * (cf.h + cf.dh * interp2);
			}
		} else {
			// Both wings walk the filter in steps of phase_inc until they run off its end.  Every lane runs the
			// same number of taps (the longest walk) in groups of four whose loads are issued together; a tap
			// beyond the end contributes x * 0, which leaves the sum as it is.
			const unsigned limit = static_cast<unsigned>(kSrcFilterLength) << 8;
			const int n_taps = static_cast<int>((limit + k.phase_inc - 1) / k.phase_inc);
			auto wing = [&](unsigned ph0, int first, int dir) {
				for (int j0 = 0; j0 < n_taps; j0 += 4) {
					SrcTap<R> cf[4];
					R xv[4], w[4];
#pragma unroll
					for (int q = 0; q < 4; ++q) {
						const unsigned ph = ph0 + static_cast<unsigned>(j0 + q) * k.phase_inc;
						const bool in = ph < limit;
						cf[q] = src_tap(in ? (ph >> 8) : 0u);
						xv[q] = s_x[(first + dir * (j0 + q)) & (XR - 1)];
						w[q] = in ? static_cast<R>(ph & 0xFFu) / R(256.0) : R(0.0);
						if (!in) cf[q] = SrcTap<R>{R(0.0), R(0.0)};
					}
#pragma unroll
					for (int q = 0; q < 4; ++q) acc += xv[q] * (cf[q].h + cf[q].dh * w[q]);
				}
			};
			wing(static_cast<unsigned>(rint(static_cast<R>(frac) * R(k.src_ratio))), base, -1);
			wing(static_cast<unsigned>(rint(static_cast<R>((~frac) & 0xFFFFu) * R(k.src_ratio))), base + 1, 1);
		}
		return static_cast<float>(acc);
	};
	auto stage_p6 = [&](int u, int c, int pass) {
		uint64_t k_lo, k_hi;
		out_range(u, c, k_lo, k_hi);
		const uint64_t ko = k_lo + static_cast<uint64_t>(pass) * 64 + lane;
		if (ko >= k_hi) return;
		s_y[u * kYr + (ko & (kYr - 1))] = src_value(u, ko);
	};

	// P7: the converter's sink (VocalTractModel5.h:497-513): DifferenceFilter<float> (y = x - x[n-2]) times the
	// output rate, unless bypassed
	// Samples leave in whole aligned blocks of 64 (256 B): the sink of chunk c emits [floor64(k_lo), floor64(k_hi)), the
	// last chunk up to k_hi, so that no cache line is written in two pieces a tick apart (the PMC write counter
	// showed 13 % more HBM write traffic than samples that way).
	float lane_peak[U];
#pragma unroll
	for (int u = 0; u < U; ++u) lane_peak[u] = 0.0f;
	auto sink_range = [&](int u, int c, uint64_t& k_lo, uint64_t& k_hi) {
		out_range(u, c, k_lo, k_hi);
		const uint64_t k_first = s_ext[u].k_first; // (a stream's launch starts where the previous one stopped, aligned or not)
		k_lo &= ~63ull;
		k_lo = k_lo > k_first ? k_lo : k_first;
		if (c != s_ext[u].nchunks - 1) {
			k_hi &= ~63ull;
			k_hi = k_hi > k_first ? k_hi : k_first;
		}
	};
	auto stage_p7 = [&](int u, int c, int pass) {
		uint64_t k_lo, k_hi;
		sink_range(u, c, k_lo, k_hi);
		const uint64_t ko = k_lo + static_cast<uint64_t>(pass) * 64 + lane;
		const float* const yr = s_y + u * kYr;
		float y = 0.0f;
		if (ko < k_hi) {
			const float v = yr[ko & (kYr - 1)];
			if (k5.bypass) {
				y = v;
			} else {
				const float v2 = ko >= 2 ? yr[(ko - 2) & (kYr - 1)] : 0.0f;
				const float d = v - v2;
				y = static_cast<float>(static_cast<R>(d) * R(k5.output_rate));
			}
			const uint64_t kout = ko - s_ext[u].k_first; // (a stream's launch numbers its samples from its own first one)
			if (kout < a.audio_stride) a.audio[GVTM_M5_UTT(u, (group * U + u)) * a.audio_stride + kout] = y;
		}
		// reduced once, after the last tick
		if (U == 1 || u == 0) lane_peak[0] = fmaxf(lane_peak[0], fabsf(y));
		else lane_peak[U - 1] = fmaxf(lane_peak[U - 1], fabsf(y));
	};

	// -------------------------------------------------------------------------------------
	// serial stages

	// A wavefront runs ONE serial role for the whole kernel, so the recurrence states of the roles share one
	// register array (each role names its own view of it) instead of each occupying registers in every wavefront.
	R st[9];
#pragma unroll
	for (int i = 0; i < 9; ++i) st[i] = R(0.0);

	// I: Controller::synthesize's interpolation (Controller.cpp:294-311), lane p owns parameter p and runs the
	// chunk its consumer pass needs next
	float ip_cur = 0.f, ip_delta = 0.f, ip_this = 0.f, ip_next = 0.f, ip_next2 = 0.f;
	uint32_t ip_j = 0;
	int ip_frame = 0;
	const int Lp = lane & 15;
	const int ip_u = lane >> 4; // lanes 16u .. 16u + 15 interpolate utterance u
	const int ip_frames = ip_u < U ? s_ext[ip_u].frames : 0;
	const int ip_last = ip_u < U ? s_ext[ip_u].last_frame : 0; // last readable row: frames - 1, or the look-ahead frame of a push
	const float* __restrict__ P = TARGETS ? nullptr : a.params + GVTM_M5_UTT(0, (group * U + (ip_u < U ? ip_u : 0))) * a.max_frames * 16;
	// I, from targets (kTargets5Flag): lane 16u + p walks the points of utterance u's list for parameter p (vtm_targets.hpp): the
	// filter's sum, the entering and the leaving value, the two cursors and the steps at which they move next.  (A refused
	// utterance and a row beyond the batch have 0 steps: their list ids and offsets are never read.)
	// A stream's launch walks absolute steps from the utterance's step_base on: behind step 0 the walk resumes on the sum the
	// previous launch left in the stream state (targets_resume; the points are the stream's log, in absolute steps), and the
	// epilogue stores the sum back.  An utterance the launch does not advance keeps its sums.
	// Under several voices (kVoices5Flag with kTargets5Flag: gvtm_synthesize_targets_model5_voices_device, and a stream's
	// gvtm_stream_push_targets_model5_voices) the utterance, and with it the slot of its lists and of its sums in the stream
	// state, is the row map's, and the filter's length and reciprocal are the
	// workgroup's voice's, a.tg_voice_N[voice] and a.tg_voice_invN[voice], read once per workgroup as vtm_kernel_v2.inc does.
	[[maybe_unused]] TargetsWalk tg{};
	[[maybe_unused]] int64_t tg_base = 0;
	[[maybe_unused]] int64_t tgv_N = 0;
	[[maybe_unused]] double tgv_invN = 0.0;
	if constexpr (TARGETS && VOICES) {
		tgv_N = a.tg_voice_N[voice];
		tgv_invN = a.tg_voice_invN[voice];
	}
	[[maybe_unused]] const auto tg_length = [&]() -> int64_t { if constexpr (VOICES) return tgv_N; else return a.tg_N; };
	[[maybe_unused]] const auto tg_inverse = [&]() -> double { if constexpr (VOICES) return tgv_invN; else return a.tg_invN; };
	if constexpr (TARGETS) {
		if (role == 3 && ip_u < U && ip_frames > 0) {
			const size_t slot = GVTM_M5_UTT(ip_u, (group * U + ip_u)) * GVTM_N_PARAM + Lp;
			const int64_t list = a.tg_ids ? static_cast<int64_t>(a.tg_ids[slot]) : static_cast<int64_t>(slot);
			if (streaming) tg_base = static_cast<int64_t>(s_ext[ip_u].step_base);
			if (tg_base > 0) {
				const double* sums = reinterpret_cast<const double*>(a.stream + GVTM_M5_UTT(ip_u, (group * U + ip_u)) * a.stream_stride + Stream5Layout::sums());
				targets_resume(tg, a.tg_steps, a.tg_values, a.tg_offsets[list], a.tg_offsets[list + 1], tg_length(), tg_base, sums[Lp]);
			} else {
				targets_begin(tg, a.tg_steps, a.tg_values, a.tg_offsets[list], a.tg_offsets[list + 1], tg_length());
			}
		}
	} else if (role == 3 && ip_u < U && ip_frames > 0) {
		ip_this = P[Lp];
		ip_next = P[static_cast<size_t>(ip_last > 1 ? 1 : ip_last) * 16 + Lp];
		ip_next2 = P[static_cast<size_t>(ip_last > 2 ? 2 : ip_last) * 16 + Lp];
	}
	auto stage_interp = [&](int t) {
		// (the resampler's output ranges: by idle lanes of this wavefront, one tick before the resampler needs them)
		if (lane >= 16 * U && lane < 16 * U + U) stage_bounds(lane - 16 * U, t - 11);
		if (ip_u >= U) return;
		const int c = t - (Lp < 3 ? 0 : (Lp < 7 ? 3 : 6));
		const int valid = valid_in(ip_u, c);
		if (valid <= 0) return;
		float* out = s_prm + ip_u * kN_prm + static_cast<size_t>(c & 1) * C * 16 + Lp;
		if constexpr (TARGETS) {
			// The second driver, as vtm_kernel_v2.inc has it: the moving average of the lane's target list, step by step, in blocks
			// of four steps.  The cursors' bookkeeping only runs for a block in which some lane's cursor moves (a point enters, or
			// leaves N steps later); every other block is four times {two double additions, a multiplication, a conversion, a
			// store}.  A partial last block runs on: no cursor passes the end of its list, and the extra rows are never read
			// (valid <= C, a multiple of four: they stay inside the chunk's slot).  The steps are absolute (tg_base: a stream's
			// step_base, else 0); the lanes of the wavefront are at different chunks by their lag, which __any covers.
			const int64_t first = tg_base + static_cast<int64_t>(c) * C;
			for (int s0 = 0; s0 < valid; s0 += 4) {
				if (__builtin_expect(__any(targets_moves(tg, first + s0, 4)), 0)) {
#pragma unroll
					for (int q = 0; q < 4; ++q) {
						targets_move(tg, first + s0 + q, a.tg_steps, a.tg_values, tg_length());
						out[(s0 + q) * 16] = targets_step(tg, tg_inverse());
					}
				} else {
#pragma unroll
					for (int q = 0; q < 4; ++q) out[(s0 + q) * 16] = targets_step(tg, tg_inverse());
				}
			}
			return;
		}
		const uint32_t cs = k.control_steps;
		const float coef = k.interp_coef;
		for (int s = 0; s < valid; ++s) {
			if (ip_j == 0) {
				ip_cur = ip_this;
				ip_delta = interp_delta(ip_next, ip_cur, coef);
			}
			out[s * 16] = ip_cur;
			ip_cur = interp_advance(ip_cur, ip_delta);
			if (++ip_j == cs) {
				ip_j = 0;
				++ip_frame;
				ip_this = ip_next;
				ip_next = ip_next2;
				const int f = ip_frame + 2;
				ip_next2 = P[static_cast<size_t>(f < ip_last ? f : ip_last) * 16 + Lp];
			}
		}
	};

	// S: the scalar recurrences.  Rosenberg phase (RosenbergBGlottalSource.h:141-147), NoiseSource, the glottal-noise
	// Butterworth1 and the frication-noise Butterworth2 (VocalTractModel5.h:549-551, :559).  Blocks of four steps,
	// the next block's inputs fetched while this one is computed; a partial last block runs on (the state is
	// never used after the utterance's last chunk); only lane 0 stores.
	// (the noise generator's seed is double in every class, NoiseSource.h:41-54: the float class keeps it beside st[])
	double seed_wide = 0.0;
	auto seed_slot = [&]() -> double& {
		if constexpr (FLOAT) return seed_wide;
		else return st[2];
	};
	R &sc_t = st[0], &sc_t2 = st[1];
	double& sc_seed = seed_slot();
	R &gn_x1 = st[3], &gn_y1 = st[4];
	R &fn_x1 = st[5], &fn_x2 = st[6], &fn_y1 = st[7], &fn_y2 = st[8];
	if (role == 1) {
		sc_t2 = R(k5.rb_t1) + R(k5.rb_tn_max); // RosenbergBGlottalSource::reset
		sc_seed = 0.7892347;                 // NoiseSource's initial seed (NoiseSource.h:32-34)
	}
	// a stream's recurrence states as the previous launch left them (a fresh stream holds the values above and zeros)
	if (streaming) {
		if (role == 1 && lane < U && GVTM_M5_UTT(lane, group * U + lane) < a.batch) {
			const double* sc = reinterpret_cast<const double*>(a.stream + GVTM_M5_UTT(lane, (group * U + lane)) * a.stream_stride + Stream5Layout::scalars());
#pragma unroll
			for (int i = 0; i < 9; ++i) st[i] = static_cast<R>(sc[kS5Scan + i]);
			if constexpr (FLOAT) seed_wide = sc[kS5Scan + 2];
		} else if (role == 2 && lane < 2 * U && GVTM_M5_UTT(lane >> 1, group * U + (lane >> 1)) < a.batch) {
			// (lane u: glottal low-pass and band-pass memories of utterance u; lanes 2u, 2u + 1: its transmitted-flow memories)
			const double* sc2 = reinterpret_cast<const double*>(a.stream + GVTM_M5_UTT(lane >> 1, (group * U + (lane >> 1))) * a.stream_stride + Stream5Layout::scalars());
			st[3] = static_cast<R>(sc2[kS5Fo + (lane & 1)]);
			if (lane < U && GVTM_M5_UTT(lane, group * U + lane) < a.batch) {
				const double* sc = reinterpret_cast<const double*>(a.stream + GVTM_M5_UTT(lane, (group * U + lane)) * a.stream_stride + Stream5Layout::scalars());
				st[0] = static_cast<R>(sc[kS5Gp]);
				st[1] = static_cast<R>(sc[kS5Bp]);
				st[2] = static_cast<R>(sc[kS5Bp + 1]);
			}
		} else if (role == 0 && lane <= kNose && GVTM_M5_UTT(tube_u, group * U + tube_u) < a.batch) {
			const double* tb = reinterpret_cast<const double*>(a.stream + GVTM_M5_UTT(tube_u, (group * U + tube_u)) * a.stream_stride + Stream5Layout::tube()) + lane * 4;
#pragma unroll
			for (int i = 0; i < 4; ++i) st[i] = static_cast<R>(tb[i]);
		}
	}
	// (lane u runs utterance u; the lanes beyond mirror the last one and store nothing)
	const int su = lane < U ? lane : U - 1;
	auto stage_s = [&](int c) {
		const int valid = valid_any(c);
		const R2* rd = reinterpret_cast<const R2*>(s_rd + su * kN_rd + static_cast<size_t>(c & 1) * (C + 4) * 2);
		R2* rst = reinterpret_cast<R2*>(s_rst + su * kN_rst + static_cast<size_t>(c & 1) * C * 2);
		R2* rn = reinterpret_cast<R2*>(s_rn + su * kN_rn + static_cast<size_t>(c & 3) * C * 2);
		const R gb0 = R(k5.gn_b0), ga1 = R(k5.gn_a1), fb0 = R(k5.fn_b0), fb1 = R(k5.fn_b1), fa1 = R(k5.fn_a1), fa2 = R(k5.fn_a2);
		R2 nx[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) nx[q] = rd[q];
		for (int s0 = 0; s0 < valid; s0 += 4) {
			R2 in[4];
#pragma unroll
			for (int q = 0; q < 4; ++q) in[q] = nx[q];
#pragma unroll
			for (int q = 0; q < 4; ++q) nx[q] = rd[s0 + 4 + q]; // the last block reads the four pad entries
			R2 ot[4], on[4];
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				ot[q] = R2{sc_t, sc_t2};
				R tn = sc_t + in[q].x;
				const bool wrap = tn > R(1.0);
				sc_t = wrap ? tn - R(1.0) : tn;
				sc_t2 = wrap ? in[q].y : sc_t2;
				sc_seed = noise_advance(sc_seed);
				const R white = static_cast<R>(sc_seed - 0.5);
				const R gn = gb0 * (white + gn_x1) - ga1 * gn_y1;
				gn_x1 = white;
				gn_y1 = gn;
				const R fn = fb0 * (white + fn_x2) + fb1 * fn_x1 - fa1 * fn_y1 - fa2 * fn_y2;
				fn_x2 = fn_x1;
				fn_x1 = white;
				fn_y2 = fn_y1;
				fn_y1 = fn;
				on[q] = R2{gn, fn};
			}
			if (lane < U) {
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					rst[s0 + q] = ot[q];
					rn[s0 + q] = on[q];
				}
			}
		}
	};

	// F: the recursive half of the glottal low-pass, pulse = u - a1 pulse[-1]
	R& gp_y1 = st[0];
	auto stage_f = [&](int c) {
		const int valid = valid_any(c);
		const R2* up = reinterpret_cast<const R2*>(s_u + su * kN_u + static_cast<size_t>(c & 1) * (C + 4));
		R2* pl = reinterpret_cast<R2*>(s_pl + su * kN_pl + static_cast<size_t>(c & 1) * C);
		const R a1 = R(k5.gp_a1);
		R2 n0 = up[0], n1 = up[1];
		for (int s0 = 0; s0 < valid; s0 += 4) {
			const R2 i0 = n0, i1 = n1;
			n0 = up[s0 / 2 + 2];
			n1 = up[s0 / 2 + 3];
			const R y0 = i0.x - a1 * gp_y1;
			const R y1 = i0.y - a1 * y0;
			const R y2 = i1.x - a1 * y1;
			const R y3 = i1.y - a1 * y2;
			gp_y1 = y3;
			if (lane < U) {
				pl[s0 / 2] = R2{y0, y1};
				pl[s0 / 2 + 1] = R2{y2, y3};
			}
		}
	};

	// Fb: the recursive half of the frication band-pass, y = ub - a1 y[-1] - a2 y[-2] (coefficients change per step)
	R &bp_y1 = st[1], &bp_y2 = st[2];
	auto stage_fb = [&](int c) {
		const int valid = valid_any(c);
		const R2* ub = reinterpret_cast<const R2*>(s_ub + su * kN_ub + static_cast<size_t>(c & 1) * (C + 4));
		const R2* a12 = reinterpret_cast<const R2*>(s_ra12 + su * kN_ra12 + static_cast<size_t>(c % 3) * (C + 4) * 2);
		R2* bp = reinterpret_cast<R2*>(s_bp + su * kN_bp + static_cast<size_t>(c & 1) * C);
		R2 n0 = ub[0], n1 = ub[1];
		R2 nc[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) nc[q] = a12[q];
		for (int s0 = 0; s0 < valid; s0 += 4) {
			const R2 i0 = n0, i1 = n1;
			R2 cf[4];
#pragma unroll
			for (int q = 0; q < 4; ++q) cf[q] = nc[q];
			n0 = ub[s0 / 2 + 2];
			n1 = ub[s0 / 2 + 3];
#pragma unroll
			for (int q = 0; q < 4; ++q) nc[q] = a12[s0 + 4 + q];
			const R y0 = i0.x - cf[0].x * bp_y1 - cf[0].y * bp_y2;
			const R y1 = i0.y - cf[1].x * y0 - cf[1].y * bp_y1;
			const R y2 = i1.x - cf[2].x * y1 - cf[2].y * y0;
			const R y3 = i1.y - cf[3].x * y2 - cf[3].y * y1;
			bp_y2 = y2;
			bp_y1 = y3;
			if (lane < U) {
				bp[s0 / 2] = R2{y0, y1};
				bp[s0 / 2 + 1] = R2{y2, y3};
			}
		}
	};

	// Fo: recursion of the transmitted flow, outT = (cT1 outT[-1] + cT2 in) + cT3 in[-1]; lane 0 the mouth (cT1 changes
	// per step), lane 1 the nose
	R& fo_y1 = st[3];
	// (lanes 2u, 2u + 1: mouth and nose of utterance u)
	const int fo_u = (lane >> 1) < U ? (lane >> 1) : U - 1;
	auto stage_fo = [&](int c) {
		const int valid = valid_any(c);
		const bool mouth = (lane & 1) == 0;
		const R* pc;
		if constexpr (FLOAT) {
			// (the nose's constant cT1 is a widened float in the constants block: the nose lane walks a narrowed copy)
			if (lane == 1) s_dump[0] = R(k5.nose_c[0]);
			pc = mouth ? s_rmo + fo_u * kN_rmo + static_cast<size_t>(c & 3) * C * 3 : s_dump;
		} else {
			pc = mouth ? s_rmo + fo_u * kN_rmo + static_cast<size_t>(c & 3) * C * 3 : &s_k5->nose_c[0];
		}
		const int c_stride = mouth ? 3 : 0;
		const R* pv = s_yv + fo_u * kN_yv + static_cast<size_t>(c & 1) * (C + 2) * 4 + (mouth ? 0 : 2);
		R* po = s_oo + fo_u * kN_oo + static_cast<size_t>(c & 1) * C * 2 + (mouth ? 0 : 1);
		R nc = pc[0];
		R2 nv = *reinterpret_cast<const R2*>(pv);
		for (int s = 0; s < valid; ++s) {
			const R c1 = nc;
			const R2 v = nv;
			nc = pc[(s + 1) * c_stride];   // (the mouth lane reads one entry past the chunk: the next slot's, never used)
			nv = *reinterpret_cast<const R2*>(pv + (s + 1) * 4);
			const R y = (c1 * fo_y1 + v.x) + v.y;
			fo_y1 = y;
			if (lane < 2 * U) po[s * 2] = y;
		}
	};

	// T: vocalTract (VocalTractModel5.h:648-730), one section per lane: S1..S30 on lanes 0..29, N1..N21 on lanes
	// 30..50.  Every link damps; a link with a junction has the coefficient k, a plain one 0.  The loop body is the
	// same arithmetic for every lane -- what distinguishes the glottis, the 3-way junction and the open ends is
	// folded into per-lane constants and per-lane record pointers:
	//   new top    = (X - kl P) dl + add,   X = Tl' + et,  P = (Tl' + B) + et
	//   new bottom = (Xb + kr Pb) d,        Xb = Br' + eb, Pb = (T + Br') + eb
	// generic lane: Tl' = left neighbour's top, Br' = right neighbour's bottom, et = eb = 0 (propagateJunction :291-296);
	// S1: Tl' = 0, kl = -glottal loss, dl = 1, add = tube input (:652); S13 / S12: et / eb = N1's bottom, k = -/+ the
	// velum coefficient; N1: Tl' = S12.top + S13.bottom (:297-303); S30, N21: Br' = the reflected flow of the
	// radiation impedance (PoleZeroRadiationImpedance::process).
	R &top = st[0], &bot = st[1];
	R &ri_in1 = st[2], &ri_outR1 = st[3]; // PoleZeroRadiationImpedance state of an end lane (reflection side)
	auto stage_tube = [&](int c) {
		const int valid = valid_in(tube_u, c);
		const R* ru = s_ru + tube_u * kN_ru + static_cast<size_t>(c & 1) * (C + 2) * kRu;
		R* ox = s_ox + tube_u * kN_ox + static_cast<size_t>(c & 1) * C * 2;
		const R d = R(k.damping);
		// record slot of the coefficient of the link on the LEFT of lane L (kRuZero: a plain damped link)
		auto slot_left = [](int L) -> int {
			switch (L) {
			case 0: return kRuLoss;
			case 3: return kRkJ; case 5: return kRkJ + 1; case 9: return kRkJ + 2; case 15: return kRkJ + 3; case 21: return kRkJ + 4; case 25: return kRkJ + 5;
			case 27: return kRkJ + 6;
			case 33: return kRkNk;
			case kThreeRight: return kRkNVl;
			case kNasalFirst: return kRkNVu;
			case 36: return kRuNasal; case 39: return kRuNasal + 1; case 42: return kRuNasal + 2; case 45: return kRuNasal + 3; case 48: return kRuNasal + 4;
			default: return kRuZero;
			}
		};
		const bool is_first = lane == 0, is_end = lane == kMouth || lane == kNose;
		// right link: the left slot of my right neighbour; S12's right side is the 3-way junction (+velum
		// coefficient); the open ends and the idle lanes have none
		const bool has_right = lane != kMouth && lane < kNose;
		const int sr = lane == kThreeLeft ? kRkVl : (has_right ? slot_left(lane + 1) : kRuZero);
		const R* pkl = ru + slot_left(lane);
		const R* pkr = ru + sr;
		const R* pe = ru + (lane == kMouth ? kRkMouth : kRuNose); // lanes in between run the nose's (stable) filter on the side
		const R* padd = ru + kRuAdd + (lane < kAddLanes ? lane : kAddLanes - 1); // what is added to my new top (0 beyond S29)
		R* pox = is_end ? ox + (lane == kNose ? 1 : 0) : s_dump + 64 + lane;
		const int ox_stride = is_end ? 2 : 0;
		const R m_t = lane == kThreeRight ? R(1.0) : R(0.0), m_b = lane == kThreeLeft ? R(1.0) : R(0.0);
		const R m_u = lane == kNasalFirst ? R(1.0) : R(0.0), nm_u = R(1.0) - m_u;
		const R d_left = is_first ? R(1.0) : d;

		// Records are fetched a pair of steps ahead into two register sets that alternate (no copies).
		struct Rec { R kl, kr, e0, e1, e2, add; };
		// read cursors at the first step of the current block of four; the offsets below are immediates
		using LdsPtr = const __attribute__((address_space(3))) R*;
		LdsPtr ckl = (LdsPtr) pkl, ckr = (LdsPtr) pkr, ce = (LdsPtr) pe, ca = (LdsPtr) padd;
		auto fetch = [&](Rec& r, int s) {
			r.kl = ckl[s * kRu];
			r.kr = ckr[s * kRu];
			LdsPtr e = ce + s * kRu;
			r.e0 = e[0]; r.e1 = e[1]; r.e2 = e[2];
			r.add = ca[s * kRu];
		};
		auto step = [&](R kl, R kr, R e0, R e1, R e2, R add, int s) {
			const R T = top, B = bot;
			const R Tl = from_left_wave(T), Br = from_right_wave(B);
			// open ends: the reflected flow outR = cR1 outR1 + cR2 in + cR3 in1 (PoleZeroRadiationImpedance::process); the
			// transmitted flow is formed downstream from the recorded input (Y, Fo)
			const R outR = e0 * ri_outR1 + e1 * T + e2 * ri_in1;
			ri_in1 = T;
			ri_outR1 = outR;
			// (the sum below is only used where there is a right link: an end lane's kr is 0)
			const R pb0 = T + Br;
			const R b30 = lane_value<kNasalFirst>(B);
			const R q11 = lane_value<kThreeLeft>(pb0); // S12.top + S13.bottom
			const R Brp = is_end ? outR : Br;
			const R et = b30 * m_t, eb = b30 * m_b;
			const R Tlp = q11 * m_u + Tl * nm_u;
			const R X = Tlp + et;
			const R Pt = (Tlp + B) + et;
			top = (X - kl * Pt) * d_left + add; // add: the tube input (S1) or my share of the frication noise (:716-726)
			const R Xb = Brp + eb;
			const R Pb = pb0 + eb;
			bot = (Xb + kr * Pb) * d;
			pox[s * ox_stride] = T;
		};
#define GVTM_M5_STEP(r, s) step(r.kl, r.kr, r.e0, r.e1, r.e2, r.add, s)
		if (valid > 0) {
			Rec a0, a1, b0, b1;
			fetch(a0, 0);
			fetch(a1, 1);
			for (int s = 0; s < valid; s += 4) {
				fetch(b0, 2);
				fetch(b1, 3);
				GVTM_M5_STEP(a0, s);
				GVTM_M5_STEP(a1, s + 1);
				fetch(a0, 4); // the last block reads the two pad records
				fetch(a1, 5);
				GVTM_M5_STEP(b0, s + 2);
				GVTM_M5_STEP(b1, s + 3);
				ckl += 4 * kRu; ckr += 4 * kRu; ce += 4 * kRu; ca += 4 * kRu;
				// keep the cursors as they are written (the loop optimiser otherwise rebases them on one counter
				// with negative offsets, which LDS instructions cannot encode: an address add per load)
				asm volatile("" : "+v"(ckl), "+v"(ckr), "+v"(ce), "+v"(ca));
			}
		}
#undef GVTM_M5_STEP
	};

	// -------------------------------------------------------------------------------------
	// the tick loop

	if (role == 0) __builtin_amdgcn_s_setprio(3);
	else if (role < 4) __builtin_amdgcn_s_setprio(1);

	const bool stamping = !VOICES && a.phase_cycles != nullptr && lane == 0;
	unsigned long long busy = 0;
	const int n_ticks = max_chunks + 14;
	for (int t = 0; t < n_ticks; ++t) {
		auto live = [&](int c) { return c >= 0 && c < max_chunks; };
		const unsigned long long t_begin = stamping ? clock64() : 0ull;
		switch (role) {
		case 0: stage_tube(t - 8); break;
		case 1: stage_s(t - 2); break;
		case 2:
			stage_f(t - 4);
			stage_fb(t - 6);
			stage_fo(t - 10);
			break;
		case 3: stage_interp(t); break;
		default: {
			// 64-lane passes the resampler and its sink need this tick (their chunks' output ranges were stored a tick ago)
			auto passes_of = [&](int u, int c) -> int {
				if (!live(c)) return 0;
				uint64_t lo, hi;
				out_range(u, c, lo, hi);
				return static_cast<int>((hi - lo + 63) / 64);
			};
			auto sink_passes_of = [&](int u, int c) -> int {
				if (!live(c)) return 0;
				uint64_t lo, hi;
				sink_range(u, c, lo, hi);
				return static_cast<int>((hi - lo + 63) / 64);
			};
			// the resampler's and the sink's passes: utterance 0's first, then utterance 1's
			const int p6_first = passes_of(0, t - 12), p7_first = sink_passes_of(0, t - 13);
			const int p6_passes = p6_first + (U > 1 ? passes_of(U - 1, t - 12) : 0);
			const int p7_passes = p7_first + (U > 1 ? sink_passes_of(U - 1, t - 13) : 0);
			const int n_passes = 8 + p6_passes + p7_passes;
			if (wave == kFirstHelper && lane == 0) s_ticket[(t + 1) & 1] = 0u; // next tick's counter (idle this tick)
			for (;;) {
				unsigned idx = 0;
				if (lane == 0) idx = atomicAdd(&s_ticket[t & 1], 1u);
				idx = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(idx)));
				if (idx >= static_cast<unsigned>(n_passes)) break;
				int ps = static_cast<int>(idx);
				const unsigned long long d0 = stamping ? clock64() : 0ull;
				int stage;
				// heaviest passes first
				if (ps == 0) {
					stage = 0;
					if (live(t - 7)) stage_a2(t - 7);
				} else if (ps == 1) {
					stage = 1;
					if (live(t - 1)) stage_a1a(t - 1);
				} else if (ps == 2) {
					stage = 2;
					if (live(t - 4)) stage_a1b(t - 4);
				} else if ((ps -= 3) < p6_passes) {
					stage = 3;
					if (live(t - 12)) {
						if (ps < p6_first) stage_p6(0, t - 12, ps);
						else stage_p6(U - 1, t - 12, ps - p6_first);
					}
				} else if ((ps -= p6_passes) == 0) {
					stage = 4;
					if (live(t - 3)) stage_b(t - 3);
				} else if (ps == 1) {
					stage = 5;
					if (live(t - 5)) stage_m(t - 5);
				} else if (ps == 2) {
					stage = 6;
					if (live(t - 7)) stage_n(t - 7);
				} else if (ps == 3) {
					stage = 7;
					if (live(t - 11)) stage_x(t - 11);
				} else if (ps == 4) {
					stage = 9;
					if (live(t - 9)) stage_y(t - 9);
				} else {
					stage = 8;
					ps -= 5;
					if (live(t - 13)) {
						if (ps < p7_first) stage_p7(0, t - 13, ps);
						else stage_p7(U - 1, t - 13, ps - p7_first);
					}
				}
				if (stamping) atomicAdd(&s_diag[stage], clock64() - d0);
			}
			break;
		}
		}
		if (stamping) busy += clock64() - t_begin;
		__syncthreads();
	}
	// SampleRateConverter's flush overrun (SampleRateConverter.h:298-308 with :462-471; see vtm_kernel_v2.inc's epilogue):
	// one more lap of the 1024-sample ring, evaluated from its final contents, the sink running on over it
	// (the two samples in front of the lap are still in the converted-sample ring)
	if (!k.upsampling && kFinal) {
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const Extent e = s_ext[u];
			uint64_t k_from = 0, k_to = 0;
			if (e.nchunks == 0 || !src_flush_overrun(k.time_inc, k.pad, e.step_base + e.steps, k_from, k_to)) continue;
			auto v_at = [&](uint64_t kk) -> float { return kk < k_from ? s_y[u * kYr + (kk & (kYr - 1))] : src_value(u, kk); };
			for (uint64_t ko = k_from + tid; ko < k_to; ko += kThreads) {
				const float v = v_at(ko);
				float y;
				if (k5.bypass) {
					y = v;
				} else {
					const float v2 = ko >= 2 ? v_at(ko - 2) : 0.0f;
					const float d = v - v2;
					y = static_cast<float>(static_cast<R>(d) * R(k5.output_rate));
				}
				if (ko - e.k_first < a.audio_stride) a.audio[GVTM_M5_UTT(u, (group * U + u)) * a.audio_stride + (ko - e.k_first)] = y;
				lane_peak[u] = fmaxf(lane_peak[u], fabsf(y));
			}
		}
	}
#pragma unroll
	for (int u = 0; u < U; ++u) {
		float lp = lane_peak[u];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) lp = fmaxf(lp, __shfl_xor(lp, off));
		if (lane == 0) atomicMax(&s_peak[u], __float_as_uint(lp));
	}
	__syncthreads();
	// diagnostics: busy cycles per wavefront (in wavefront order; see role mapping above), then per helper stage
	if (stamping && wave < 7) a.phase_cycles[group * 16 + wave] = busy;
	__syncthreads();
	if (!VOICES && a.phase_cycles != nullptr && tid < 9) a.phase_cycles[group * 16 + 7 + tid] = s_diag[tid];

	if (tid < U) {
		const size_t ug = GVTM_M5_UTT(tid, group * U + tid);
		if (ug < a.batch) {
			if (a.maxabs) a.maxabs[ug] = __uint_as_float(s_peak[tid]);
			const Extent e = s_ext[tid];
			const uint64_t total = e.step_base + e.steps;
			const uint64_t k_end = kFinal ? src_output_count(k.time_inc, k.pad, k.upsampling, total) : ((total << 16) + k.time_inc - 1) / k.time_inc;
			if (a.out_counts) a.out_counts[ug] = static_cast<int64_t>(k_end - e.k_first);
		}
	}

	// ---- a stream's states for the next launch
	if (streaming) {
		if constexpr (TARGETS) {
			// the moving averages' sums of every utterance the launch advanced, push and finish alike (a push synthesizes a
			// multiple of four steps, so no lane has run on into a partial block when its sum is stored)
			if (role == 3 && ip_u < U && ip_frames > 0) {
				double* sums = reinterpret_cast<double*>(a.stream + GVTM_M5_UTT(ip_u, (group * U + ip_u)) * a.stream_stride + Stream5Layout::sums());
				sums[Lp] = tg.sum;
			}
		}
		if (role == 1 && lane < U && GVTM_M5_UTT(lane, group * U + lane) < a.batch) {
			double* sc = reinterpret_cast<double*>(a.stream + GVTM_M5_UTT(lane, (group * U + lane)) * a.stream_stride + Stream5Layout::scalars());
#pragma unroll
			for (int i = 0; i < 9; ++i) sc[kS5Scan + i] = st[i];
			if constexpr (FLOAT) sc[kS5Scan + 2] = seed_wide;
		} else if (role == 2 && lane < 2 * U && GVTM_M5_UTT(lane >> 1, group * U + (lane >> 1)) < a.batch) {
			double* sc2 = reinterpret_cast<double*>(a.stream + GVTM_M5_UTT(lane >> 1, (group * U + (lane >> 1))) * a.stream_stride + Stream5Layout::scalars());
			sc2[kS5Fo + (lane & 1)] = st[3];
			if (lane < U && GVTM_M5_UTT(lane, group * U + lane) < a.batch) {
				double* sc = reinterpret_cast<double*>(a.stream + GVTM_M5_UTT(lane, (group * U + lane)) * a.stream_stride + Stream5Layout::scalars());
				sc[kS5Gp] = st[0];
				sc[kS5Bp] = st[1];
				sc[kS5Bp + 1] = st[2];
			}
		} else if (role == 0 && lane <= kNose && GVTM_M5_UTT(tube_u, group * U + tube_u) < a.batch) {
			double* tb = reinterpret_cast<double*>(a.stream + GVTM_M5_UTT(tube_u, (group * U + tube_u)) * a.stream_stride + Stream5Layout::tube()) + lane * 4;
#pragma unroll
			for (int i = 0; i < 4; ++i) tb[i] = st[i];
		}
		for (int u = 0; u < U; ++u) {
			if (GVTM_M5_UTT(u, group * U + u) >= a.batch) break;
			const Extent e = s_ext[u];
			unsigned char* sb = a.stream + GVTM_M5_UTT(u, (group * U + u)) * a.stream_stride;
			double* ring = reinterpret_cast<double*>(sb + Stream5Layout::ring());
			for (int i = tid; i < XR; i += kThreads) ring[i] = s_x[u * XR + i];
			float* yr = reinterpret_cast<float*>(sb + Stream5Layout::yring());
			for (int i = tid; i < kYr; i += kThreads) yr[i] = s_y[u * kYr + i];
			if (tid == 0) {
				StreamHeader* h = reinterpret_cast<StreamHeader*>(sb);
				h->step_base = e.step_base + e.steps;
				h->peak_bits = s_peak[u];
				if (e.steps > 0) {
					// the last values of the last chunk (a push synthesizes a multiple of four steps, so its last chunk holds at least four)
					double* sc = reinterpret_cast<double*>(sb + Stream5Layout::scalars());
					const int lc = e.nchunks - 1;
					const int vl = static_cast<int>(e.steps) - lc * C;
					sc[kS5ValLast] = s_val[u * kN_val + (lc & 1) * C + vl - 1];
					sc[kS5FnmLast] = vl >= 2 ? s_fnm[u * kN_fnm + (lc & 1) * C + vl - 2] : 0.0;
					sc[kS5FnmLast + 1] = s_fnm[u * kN_fnm + (lc & 1) * C + vl - 1];
					sc[kS5Carry] = s_carry[u * kN_carry + (lc & 1) * 2];
					sc[kS5Carry + 1] = s_carry[u * kN_carry + (lc & 1) * 2 + 1];
				}
			}
		}
	}
#undef GVTM_M5_UTT
}

} // namespace m5

// LDS bytes of a workgroup of shape (FLOAT, INDEX)
template <bool FLOAT, int INDEX, bool TARGETS = false>
static size_t m5_lds_bytes()
{
	constexpr M5Shape s = m5_shape_of(FLOAT, INDEX, TARGETS);
	return m5::Offsets<s.chunk, kM5Ring, s.rows, std::conditional_t<FLOAT, float, double>, TARGETS>().total;
}

// The launch of shape (FLOAT, INDEX).  VOICES: a launch of several voices (the kernel's kVoices5Flag; args.row_map is
// set), a one-utterance shape only (the double class's, either of the float class's); `batch` is then the number of
// workgroups.  TARGETS: a launch from parameter targets (the kernel's kTargets5Flag; args.tg_offsets is set), in the shape
// (FLOAT, INDEX) of m5_targets_shape; with VOICES (vtm_kernels_m5tv.hip, vtm_kernels_m5ftv.hip) in its one-utterance shapes
template <bool FLOAT, int INDEX, bool VOICES = false, bool TARGETS = false>
static hipError_t launch_synth5_shape(const SynthArgs& args, size_t batch, hipStream_t stream)
{
	constexpr M5Shape s = m5_shape_of(FLOAT, INDEX, TARGETS);
	static_assert(!VOICES || s.rows == 1, "the voice variant has the one-utterance shapes only");
	static_assert(!(VOICES && TARGETS) || s.rows == 1, "the targets variant under several voices has the one-utterance shapes only");
	auto fn = m5::vtm5_synth_kernel<s.chunk, s.helpers, kM5Ring,
			s.rows | (VOICES ? m5::kVoices5Flag : 0) | (FLOAT ? m5::kFloat5Flag : 0) | (TARGETS ? m5::kTargets5Flag : 0)>;
	const size_t lds = m5_lds_bytes<FLOAT, INDEX, TARGETS>();
	hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(VOICES ? batch : (batch + s.rows - 1) / s.rows)), dim3(s.waves * 64), lds, stream, args);
	return hipGetLastError();
}
