// The synthesis kernel of VocalTractModel0 / 2 / 4: wave-specialised, software-pipelined over chunks.
// Included by vtm_kernels.hip inside namespace gvtm.
//
// A workgroup owns U utterances (one 16-lane DPP row each in the serial wavefronts) and eight
// wavefronts with fixed roles:
//
//   wave 0      T   the waveguide proper: one lane per tube section, nothing else in its loop
//   wave 1      S   oscillator phase recurrence + noise generator (the fp64 scalar scans)
//   wave 2      F1  IIRs BEFORE the tube: band-pass -> per-section injection, throat low-pass
//   wave 3      F2  IIRs AFTER the tube (outside its feedback loop): mouth/nose radiation
//                   high-pass, their sum, + throat -> internal-rate ring
//   wave 4      I   parameter interpolation: one lane per parameter, the float32 running sum of
//                   Controller::synthesize, each lane running the chunk its consumer needs next
//   waves 5..   H   NH helpers sharing a static list of parallel passes (per step / per output sample)
//
// Time is cut into chunks of C internal steps; every stage works on a different chunk in the
// same tick, ONE workgroup barrier per tick, and every LDS buffer has a single writer stage and
// as many slots as its readers lag:
//
//   tick c-2  I  pitch/glotVol/aspVol of chunk c (other lanes: fric* of c-3, radii of c-4) -> prm
//   tick c-1  H  P2a(c)  pitch/glotVol/aspVol -> phase increment, ax, ah1
//   tick c    S  S1(c)   phase recurrence (2 half steps) + noise                 -> pos, noise
//   tick c+1  H  P4a(c)  wavetable lookup + lerp at the 2x rate                   -> w
//   tick c+2  H  P4b(c)  FIR decimator, breathiness / cross-mix                   -> u, sig, thr
//             H  P2c(c)  fricVol/Pos/CF/BW -> taps, band-pass design              -> fr
//   tick c+3  F  F1(c)   band-pass, injection per section, throat                 -> inj, thy
//             H  P2b(c)  r1..r8, velum -> junction coefficients                   -> kl
//   tick c+4  T  tube(c)                                                          -> ox (mouth, nose)
//   tick c+5  F  F2(c)   radiation filters, sum, + throat                         -> x ring
//   tick c+6  H  P6(c)   sample-rate conversion, one lane per output sample       -> HBM
//

namespace v2 {

namespace {

// Per-step records in LDS are arrays of structures: the serial wavefronts read one step's fields side by side (lane =
// field), the helper passes write them with lane = step.  LDS has 32 banks of 4 bytes (64 for 8-byte accesses): with an
// EVEN record length the helper lanes pile onto a few banks (16 floats per record: all 32 lanes of a group on TWO banks),
// and with a distance of a multiple of 32 elements between two utterances' records the rows of a serial wavefront
// collide pairwise.  rocprofv3 on the round-1 layout: SQ_LDS_BANK_CONFLICT = 51 % of SQ_LDS_IDX_ACTIVE with four
// utterances per workgroup, the LDS busy 70 % of the time (profiles/r02_pmc_lds_*).  So: odd record lengths, and the
// records of consecutive utterances 16 (mod 32) elements apart.
constexpr int kPrm = 17; // per-step interpolated parameters (16 used)
// what the pre-tube filter wavefront consumes per step, as PLANES of C values (it reads them four steps at a time, the
// helper passes write them with lane = step): tube input, band-pass input, throat input (from the source mix) and the
// band-pass coefficients b0, a1, a2 (from the frication pass)
constexpr int kF1Planes = 6;
constexpr int kF1U = 0, kF1Sig = 1, kF1Thr = 2, kF1B0 = 3, kF1A1 = 4, kF1A2 = 5;
constexpr int kKl = 11;  // per-step tube record: J1..J7, J8 (mouth), NJ1, alpha_lr, alpha_u
constexpr int kKlK8 = 7, kKlNk1 = 8, kKlAlr = 9, kKlAu = 10;
constexpr int kInj = 9;  // per-step injection record: tube input, FC1..FC8 * frication
// Float, 10+6 tube: LANE-INDEXED tube record.  Entry L is the junction coefficient on the left of section lane L -- the
// ones that never change (0, -1 for the tube input, the fixed nasal junctions) are written once at kernel start, the pass
// that forms the coefficients only touches the others -- entry 16 is a zero, then alpha_lr, alpha_u and the mouth
// coefficient.  Every tube lane then reads {its own coefficient, its right neighbour's} as ONE two-address read at its
// lane's offset, its 3-way / mouth coefficient at a second per-lane offset and its injection (a zero entry for sections
// that get none) at a third, all three cursors advancing by the same constant: immediate offsets inside a block of
// steps, no per-step address arithmetic, no cross-lane move and sign flip for the neighbour's coefficient (12 of the
// tube wavefront's 33 vector instructions per step were such overhead).
template <typename CT, int LAYOUT>
constexpr bool lane_rec()
{
	return sizeof(CT) == 4 && LAYOUT == 0;
}
// lane-indexed tube record: 16 coefficients, a zero, alpha_lr, alpha_u, the mouth coefficient, the nose coefficient (a
// constant, so that both open ends find their reflection coefficient through the same cursor), and the nine injection
// values of the step (written by the pre-tube filter wavefront), one pad: 31 entries (odd, and in the block layout a block
// of four steps is 124 elements = 28 mod 32 banks: eight consecutive blocks start on eight different bank groups)
constexpr int kLrZero = 16, kLrAlr = 17, kLrAu = 18, kLrK8 = 19, kLrKn = 20, kLrInj = 21, kLrLen = 31;
constexpr int kl_len(bool lr)
{
	return lr ? kLrLen : kKl;
}
// Per-step frication taps, two forms.  Dense (float): taps[8], 0 (a pre-tube filter lane reads its tap, the others the
// zero).  Compact (double): at most two neighbouring sections receive frication noise (VocalTractModel0.h:524-552), so
// the record holds {share of section q, share of section q + 1, 0, q, pad} and a filter lane reads entry
// min(its section - q, 2) (unsigned: sections in front of q wrap to the zero as well): less LDS for four utterances
// in double, which is what lets them keep a chunk of 32 steps.  (Selecting with compares or with 0 / 1 weights
// instead of the indexed read made the filter wavefront the longest role: 279 -> 362 / 460 cycles per step.)
template <typename CT>
constexpr bool fr_compact()
{
	return sizeof(CT) == 8;
}
template <typename CT>
constexpr int fr_len()
{
	return fr_compact<CT>() ? 5 : 9;
}
constexpr int kFrTapA = 0, kFrTapB = 1, kFrZero = 2, kFrFirst = 3;  // compact form (kFrFirst: an int in the slot's low word)
// Where utterance u's C records of slot `slot` start (in elements).  The rows of a 32-lane group (utterances 0 | 1 and
// 2 | 3) must lie 16 (mod 32) elements apart: where C * rec is not, the second row of each pair is pushed back.
template <int C>
constexpr int rec_pad(int rec)
{
	return ((16 - (C * rec) % 32) + 32) % 32;
}
template <int C, int U>
constexpr int rec_slot(int rec) // elements of one slot (all U utterances)
{
	return U * C * rec + rec_pad<C>(rec) * ((U + 1) / 2);
}
template <int C, int U>
__host__ __device__ constexpr size_t rec_at(int rec, int slot, int u)
{
	return static_cast<size_t>(slot) * rec_slot<C, U>(rec) + static_cast<size_t>(u) * (C * rec) + static_cast<size_t>(rec_pad<C>(rec)) * ((u + 1) / 2);
}
constexpr int kDump = 64 * 4;  // doubles: [4][64], lane-contiguous so that dump stores never bank-conflict
// The internal-rate ring carries a MIRROR of its first kXMirror samples behind its end: the up-sampling resampler reads
// the 26 samples around its position as one run from the wrapped start with immediate offsets (no index arithmetic per
// tap), which may run past the ring's end by 25.
constexpr int kXMirror = 32;
constexpr int kWPre = 48;    // FIR pre-roll in front of every w slot (>= fir_taps - 1; checked on the host)
static_assert(kWPre == kStreamPreRoll, "a stream state carries one pre-roll");

struct Extent {
	int frames;       // control frames this launch synthesizes for the utterance (0 = none)
	int nchunks;      // chunks they span (0 = slot unused)
	uint32_t steps;   // internal steps of this launch
	int last_frame;   // last readable row of the utterance's frames: frames - 1, or frames when a stream's push left the
	                  // NEXT frame behind it (the interpolation's target, Controller.cpp:297-300)
	unsigned long long step_base; // internal steps synthesized by earlier launches of the stream (0: one-shot)
	unsigned long long k_first;   // first output sample of this launch = ceil(step_base * 2^16 / time_inc)
};

// Diagnostic instruments (never set in the product build; tools/build_variant.sh <name> -D... is the Makefile's recipe with them):
//   GVTM_KERNEL_TAPS  per-step intermediate values to SynthArgs::debug_taps (tests/tools/debug_taps.py); costs the serial
//                     loops their scheduling
//   GVTM_TUNE_SKIP    bit mask of stages left out, for counting instructions per stage (tools/collect_skip_counts.sh): a
//                     skipped stage leaves garbage behind
//   GVTM_TUNE_TRACE   first of two ticks whose timeline workgroup 0 records (tests/tools/tick_trace.py)
//   GVTM_TUNE_PLAN_TABLES  which single-voice float shapes read the plan's resampler phase table (bit 0) and its
//                     static-wavetable flag (bit 1), in place of the selectors' own choice (src_phase_table() below)
//   GVTM_TUNE_FILTER_SPLIT  which float shapes run the feed-forward half of the post-tube filters 64 steps at a time
//                     (bit 0), in place of the selector's own choice (filter_split_f2() below)
// The design alternatives that were measured and lost (packed resampler rows, coefficient table in device memory, tickets
// requested ahead / by position, a second pass list for the tube's idle time, role placement by SIMD, ...) are recorded in
// DESIGN.md's A/B table, not kept here.
#ifndef GVTM_KERNEL_TAPS
#define GVTM_KERNEL_TAPS 0
#endif
#ifndef GVTM_TUNE_SKIP
#define GVTM_TUNE_SKIP 0
#endif
#ifndef GVTM_TUNE_TRACE
#define GVTM_TUNE_TRACE 0
#endif
#ifndef GVTM_TUNE_PLAN_TABLES
#define GVTM_TUNE_PLAN_TABLES (-1)
#endif
#ifndef GVTM_TUNE_FILTER_SPLIT
#define GVTM_TUNE_FILTER_SPLIT (-1)
#endif
// serial wavefronts that finish their stage early join the helpers for the rest of the tick: bit 1 scan, bit 3 post-tube
// filters, bit 4 interpolation
constexpr unsigned kSerialHelpMask = 0x1a;
// resampler table kept as h only (delta formed on the fly) for an fp64 resampler with several rows: 26 KB less
template <typename CT, typename ST, int U>
constexpr bool kSrcHOnly = sizeof(ST) == 8 && U > 1;
template <typename CT, typename ST, int U, int C>
struct Smem { // (pointers only: the same for both record forms)
	DeviceConstants* kc; // copy of the plan constants
	Extent* ext;         // [U]
	CT* wavetable;   // [512]
	CT* fir;         // [kMaxFirTaps]
	SrcTap<ST>* src;     // [3328] {h, dh} pairs; fp64 resampler with several rows: h only, as ST[3328 + 1] with a
	                     // trailing 0, dh[i] = h[i+1] - h[i] formed on the fly exactly as initializeFilter did: 26 KB
	                     // less, which buys a chunk of 48 for two rows (one row measured 5 % slower that way)
	float* prm;          // [2][U][C][16]  interpolated parameters (slot = chunk parity of the writing lane)
	CT* inc;         // [2][U][C]
	CT* amp;         // [4][U][C][2]   ax, ah1
	CT* pos;         // [2][U][2C]
	CT* noise;       // [3][U][C]
	CT* w;           // [3][U][kWPre + 2C]
	CT* usg;         // [2][U][kF1Planes][C]  tube / band-pass / throat input, band-pass b0 a1 a2
	CT* fr;          // [2][U][C][kFr]
	CT* kl;          // [2][U][C][kKl]
	CT* inj;         // [2][U][C][kInj]
	CT* lanec;       // [64] per-lane constant junction coefficient (lanes whose left junction is fixed), [64] = 0;
	                 // [66..] as ints: the tube layout's LaneSpec of lane i, packed (the table itself sits in constant memory:
	                 // reading it there cost the tube wavefront ~800 cycles at the start of every tick)
	CT* thy;         // [3][U][C]      throat output
	CT* ox;          // [2][U][C][2]   mouth / nose radiation-filter inputs
	CT* opk;         // [3][U][C]      lane-indexed tube record only: 1 + mouth coefficient (the post-tube filters scale the mouth's top with it)
	ST* x;               // [U][xr]        internal-rate ring; xr (a power of two) is chosen at launch, so the ring is the
	                     //                LAST region: every other offset is a compile-time constant
	unsigned* peak;      // [U] max|y| as float bits
	unsigned long long* kb; // [2][U + 1] first output index of a chunk and one-past-last per utterance, by tick parity
	unsigned* ticket;    // [2] pass ticket counters of the helper wavefronts (by tick parity); [2], [3]: src_bounds_step() of the
	                     // plan's time_inc and this kernel's chunk (stage_bounds, where it goes by running remainder)
	unsigned long long* diag; // [8] cycles per helper stage (diagnostics)
	CT* dump;        // [kDump] sink for lanes whose result is not needed (keeps the serial loops branch-free)
};

// Byte offsets of the LDS regions (shared by the device-side carve and the host-side size query).
template <typename CT, typename ST, int U, int C, bool LR>
struct SmemOffsets {
	size_t kc, ext, wavetable, fir, src, prm, inc, amp, pos, noise, w, usg, fr, kl, inj, lanec, thy, ox, opk, peak, kb, ticket, diag, dump, x, fixed;
	__host__ __device__ constexpr SmemOffsets()
		: kc(0), ext(0), wavetable(0), fir(0), src(0), prm(0), inc(0), amp(0), pos(0), noise(0), w(0), usg(0), fr(0), kl(0),
		  inj(0), lanec(0), thy(0), ox(0), opk(0), peak(0), kb(0), ticket(0), diag(0), dump(0), x(0), fixed(0)
	{
		size_t off = 0;
		auto take = [&](size_t bytes) {
			const size_t at = off;
			off += (bytes + 15) & ~size_t(15);
			return at;
		};
		kc = take(sizeof(DeviceConstants));
		ext = take(sizeof(Extent) * U);
		wavetable = take(sizeof(CT) * kWavetableLength);
		fir = take(sizeof(CT) * kMaxFirTaps);
		src = take(kSrcHOnly<CT, ST, U> ? sizeof(ST) * (kSrcFilterLength + 1) : sizeof(SrcTap<ST>) * kSrcFilterLength);
		prm = take(sizeof(float) * 2 * rec_slot<C, U>(kPrm));
		inc = take(sizeof(CT) * 2 * U * C);
		amp = take(sizeof(CT) * 4 * U * C * 2);
		pos = take(sizeof(CT) * 2 * U * 2 * C);
		noise = take(sizeof(CT) * 3 * U * C);
		w = take(sizeof(CT) * 3 * U * (kWPre + 2 * C));
		usg = take(sizeof(CT) * 2 * rec_slot<C, U>(kF1Planes));
		fr = take(sizeof(CT) * 2 * rec_slot<C, U>(fr_len<CT>()));
		kl = take(sizeof(CT) * 2 * rec_slot<C, U>(kl_len(LR)));
		inj = take(LR ? 16 : sizeof(CT) * 2 * rec_slot<C, U>(kInj));
		lanec = take(sizeof(CT) * 72 + sizeof(int) * 64);
		thy = take(sizeof(CT) * 3 * U * C);
		ox = take(sizeof(CT) * 2 * U * C * 2);
		opk = take(LR ? sizeof(CT) * 3 * U * C : 16);
		peak = take(sizeof(unsigned) * U);
		kb = take(sizeof(unsigned long long) * 2 * (U + 1));
		ticket = take(sizeof(unsigned) * 4);
		diag = take(sizeof(unsigned long long) * 8);
		dump = take(sizeof(CT) * kDump);
		x = off;
		fixed = off;
	}
};

// LDS bytes of a workgroup whose internal-rate rings hold xr samples each
template <typename CT, typename ST, int U, int C, bool LR>
inline size_t smem_bytes(int xr)
{
	return SmemOffsets<CT, ST, U, C, LR>().fixed + ((sizeof(ST) * U * static_cast<size_t>(xr + kXMirror) + 15) & ~size_t(15));
}

// ---------------------------------------------------------------------------------------------
// Tube layouts: which section a lane of the tube wavefront is, and what sits on its two sides.
//
//   layout 0  VocalTractModel0/2: S1..S10 on lanes 0..9, N1..N6 on lanes 10..15 (one DPP row, so up to
//             four utterances per wavefront); every link damps.
//   layout 1  VocalTractModel4: S1..S30 on lanes 0..29, N1..N18 on lanes 30..47 (one utterance per
//             wavefront, neighbours fetched with wave-wide DPP shifts); scattering and damping only at
//             region boundaries, plain copies inside a region (VocalTractModel4.h:296-300, :671-745).
//
// Link kinds between a section and its RIGHT neighbour:
enum LinkKind : signed char {
	kCopy = 0,     // right.top = left.top, left.bottom = right.bottom
	kDelay = 1,    // the same with damping (VocalTractModel2.h:251-254)
	kJunction = 2, // 2-port scattering junction with damping
	kThreeWay = 3, // left side of the 3-way junction (the other partner is the first nasal section)
	kEnd = 4       // open end: reflection low-pass, radiation
};

struct LaneSpec {
	signed char link_right; // LinkKind towards the right neighbour
	signed char kl_slot;    // record slot of the junction coefficient on my LEFT, -1 = fixed (see kl_fixed)
	signed char kl_fixed;   // when kl_slot < 0: 0 -> 0.0, 1 -> -1.0 (tube input), 2.. -> nasal_k[kl_fixed - 1]
	signed char damp_left;  // my top is damped (everything but a plain copy on my left)
	signed char inj_slot;   // injection record slot added to my top, -1 = none
};

template <int LAYOUT>
struct TubeLayout;

template <>
struct TubeLayout<0> {
	static constexpr int kLanes = 16;
	static constexpr int kThreeWayLeft = 3, kThreeWayRight = 4, kNasalFirst = 10, kMouth = 9, kNose = 15;
	static constexpr bool kWaveWide = false;
	__device__ static LaneSpec lane(int L)
	{
		//                       link_right  kl_slot kl_fixed damp inj
		constexpr LaneSpec t[16] = {
			{kJunction, -1, 1, 1, 0},  // S1   top = bottom * d + input
			{kJunction, 0, 0, 1, -1},  // S2   J1 on my left
			{kJunction, 1, 0, 1, 1},   // S3   J2, FC1
			{kThreeWay, 2, 0, 1, 2},   // S4   J3, FC2; 3-way on my right
			{kJunction, -1, 0, 1, 3},  // S5   3-way on my left, FC3
			{kDelay, 3, 0, 1, 4},      // S6   J4, FC4; S6|S7 share a region
			{kJunction, -1, 0, 1, 5},  // S7   FC5
			{kJunction, 4, 0, 1, 6},   // S8   J5, FC6
			{kJunction, 5, 0, 1, 7},   // S9   J6, FC7
			{kEnd, 6, 0, 1, 8},        // S10  J7, FC8; mouth
			{kJunction, -1, 0, 1, -1}, // N1   3-way on my left
			{kJunction, kKlNk1, 0, 1, -1}, // N2  NJ1 (velum | nasal_radius_1)
			{kJunction, -1, 2, 1, -1}, // N3   fixed nasal junctions
			{kJunction, -1, 3, 1, -1}, // N4
			{kJunction, -1, 4, 1, -1}, // N5
			{kEnd, -1, 5, 1, -1},      // N6   nose
		};
		return t[L & 15];
	}
};

template <>
struct TubeLayout<1> {
	static constexpr int kLanes = 48;
	static constexpr int kThreeWayLeft = 11, kThreeWayRight = 12, kNasalFirst = 30, kMouth = 29, kNose = 47;
	static constexpr bool kWaveWide = true;
	__device__ static LaneSpec lane(int L)
	{
		constexpr LaneSpec c = {kCopy, -1, 0, 0, -1}; // section inside a region: copy on both sides
		constexpr LaneSpec t[48] = {
			{kCopy, -1, 1, 1, 0},       // S1   tube input
			c,                           // S2
			{kJunction, -1, 0, 0, -1},  // S3   J1 on my right
			{kCopy, 0, 0, 1, -1},       // S4   J1 on my left
			{kJunction, -1, 0, 0, -1},  // S5   J2 on my right
			{kCopy, 1, 0, 1, 1},        // S6   J2, FC1
			c, c,                        // S7 S8
			{kJunction, -1, 0, 0, -1},  // S9   J3 on my right
			{kCopy, 2, 0, 1, 2},        // S10  J3, FC2
			c,                           // S11
			{kThreeWay, -1, 0, 0, -1},  // S12  3-way on my right
			{kCopy, -1, 0, 1, 3},       // S13  3-way on my left, FC3
			c,                           // S14
			{kJunction, -1, 0, 0, -1},  // S15  J4 on my right
			{kCopy, 3, 0, 1, 4},        // S16  J4, FC4
			c,                           // S17
			{kDelay, -1, 0, 0, -1},     // S18  damped link to S19
			{kCopy, -1, 0, 1, 5},       // S19  FC5
			c,                           // S20
			{kJunction, -1, 0, 0, -1},  // S21  J5 on my right
			{kCopy, 4, 0, 1, 6},        // S22  J5, FC6
			c, c,                        // S23 S24
			{kJunction, -1, 0, 0, -1},  // S25  J6 on my right
			{kCopy, 5, 0, 1, 7},        // S26  J6, FC7
			{kJunction, -1, 0, 0, -1},  // S27  J7 on my right
			{kCopy, 6, 0, 1, 8},        // S28  J7, FC8
			c,                           // S29
			{kEnd, -1, 0, 0, -1},       // S30  mouth
			{kCopy, -1, 0, 1, -1},      // N1   3-way on my left
			c,                           // N2
			{kJunction, -1, 0, 0, -1},  // N3   NJ1 on my right
			{kCopy, kKlNk1, 0, 1, -1},  // N4   NJ1
			c,                           // N5
			{kJunction, -1, 0, 0, -1},  // N6
			{kCopy, -1, 2, 1, -1},      // N7   NJ2 (fixed)
			c,                           // N8
			{kJunction, -1, 0, 0, -1},  // N9
			{kCopy, -1, 3, 1, -1},      // N10  NJ3
			c,                           // N11
			{kJunction, -1, 0, 0, -1},  // N12
			{kCopy, -1, 4, 1, -1},      // N13  NJ4
			c,                           // N14
			{kJunction, -1, 0, 0, -1},  // N15
			{kCopy, -1, 5, 1, -1},      // N16  NJ5
			c,                           // N17
			{kEnd, -1, 0, 0, -1},       // N18  nose
		};
		return t[L < 48 ? L : 47];
	}
};

} // namespace

// G = wavefronts per serial role: a wavefront serves up to four utterances (DPP rows), so a workgroup of
// U = 8 runs two tube / scan / filter / interpolation wavefronts side by side (two independent recurrence
// chains per compute unit) on one set of tables, one barrier and one helper pool.
// The 48-section tube fills a wavefront: a workgroup of U utterances then has U tube wavefronts (wavefronts
// 0 .. U-1) and ONE wavefront for each of the other serial roles, which still serve an utterance per DPP row.
template <int U, int LAYOUT>
constexpr int serial_waves()
{
	return TubeLayout<LAYOUT>::kWaveWide ? U + 4 : 5 * ((U + 3) / 4);
}

// Several voices in one launch (gvtm_synthesize_voices_device): the kernel's last template argument carries, besides the tube
// layout in bit 0, the flag kVoicesFlag (default off).  With it, workgroup g synthesizes the utterances
// a.row_map[g * U .. g * U + U) (-1: an empty row, only ever at the end of a group) of voice a.group_voice[g] (-1: a group past
// the last voice's, which exits at once), and that voice picks the constants a.kconst[voice], the wavetable at
// a.wavetable + voice * 512 and the ring length (a stream's: that of the voice's single-voice stream); the LDS is sized for
// the longest ring of the launch (the ring is the last region).  Without the flag every expression below is the one it was before the flag existed: each voice-dependent one is
// a conditional on the constant VOICES whose voice arm the compiler never emits, so the single-voice kernels compile to
// the same code.  (A separate bool parameter would rename every kernel, a wrapper kernel around an inlined body changes
// what the register allocator spills: float, eight rows 476 -> 620 bytes of scratch.)
constexpr int kVoicesFlag = 2;
// Synthesis from parameter targets (gvtm_synthesize_targets_device): a third bit of the same argument, kTargetsFlag (default
// off).  With it the interpolation wavefront has a second driver: lane L of row u walks the points of list
// a.tg_ids[16 utt + L] through the moving average of vtm_targets.hpp and writes the same float per step into the `prm`
// record; an utterance is a.frame_counts[utt] STEPS long, and there are no frames.  Together with kVoicesFlag
// (gvtm_synthesize_targets_voices_device; vtm_kernels_targets_voices.hip) utt is the row map's, and the filter's length
// and reciprocal are the workgroup's voice's, a.tg_voice_N[voice] and a.tg_voice_invN[voice].  On behalf of a stream
// (gvtm_stream_push_targets) the steps are absolute and the filters' sums travel in the stream state.  Nothing else differs between the two
// drivers, and as with kVoicesFlag every difference is a conditional on the constant TARGETS whose targets arm the
// compiler never emits for the other kernels.
constexpr int kTargetsFlag = 4;

__device__ __forceinline__ size_t voice_row(const SynthArgs& a, size_t slot)
{
	const int r = a.row_map[slot];
	return r < 0 ? a.batch : static_cast<size_t>(r);
}

// which shapes keep the library fallbacks of the float routines in their passes, and which take their plan constants as
// floats from the kernel arguments (SynthArgs::fir_k: the host fills the block for every float plan, launch_v2 checks it)
template <int D, int U> constexpr bool far_calls_inline() { return D == 1 && U == 4; }
// which float shapes take the decimator's coefficients as literals (kGlottalFirF32) in their unrolled tap loop; the others
// keep them in SGPRs (kernel arguments, SynthArgs::fir_k.f).  Literals for every shape, parent / literals, kernel ms, three
// interleaved runs each, 500 frames (profiles/fir_literals_ab.md): four rows SectionDelay 2 (x 7500) 335.5 / 319.7 and
// SectionDelay 1 12.247 / 11.819; one row SectionDelay 2 4.518 / 4.490; but two rows SectionDelay 2 4.777 / 4.793 and one row
// SectionDelay 1 2.420 / 2.440, each slower by a little more than the parent's spread (0.015, 0.017): those two keep the SGPRs.
template <int D, int U> constexpr bool fir_literal_taps() { return !((D == 1 && U == 1) || (D == 2 && U == 2)); }
// which shapes carry the resampler's output ranges from tick to tick by running remainder (src_bounds_advance,
// csrc/vtm_design.hpp) instead of dividing them out every tick (stage_bounds).  The kernel answers to any change of its
// helper loop's registers, so this too went by measurement, shape by shape (profiles/bounds_recurrence_ab.md; parent / running
// remainder, kernel ms, three interleaved runs each, 4096 utterances): float, four rows, SectionDelay 2 (x 7500 frames)
// 320.68 / 317.80 and SectionDelay 3 (x 500) 56.07 / 54.14 take it; SectionDelay 1 11.896 / 11.917, SectionDelay 4 95.13 / 95.42,
// two rows (512 utterances) SectionDelay 2 4.797 / 4.790 and SectionDelay 1 2.579 / 2.578, fp64 (x 1000) 77.91 / 77.94 and mixed
// 73.84 / 83.77 do not gain or lose, and keep the divisions and the parent's instruction stream; so does the 48-lane layout,
// which was not measured.
template <typename CT, int D, int U, int LAYOUT> constexpr bool bounds_by_recurrence() { return sizeof(CT) == 4 && U == 4 && LAYOUT == 0 && (D == 2 || D == 3); }
// which float shapes take what a plan fixes from the plan instead of forming it in every pass: the resampler's 26
// coefficients of an output phase from the plan's table in device memory (SynthArgs::src_phase; vtm_design.hpp:
// design_src_phase_table) and "the wavetable is static" from one uniform flag (SynthArgs::static_wavetable).  Adopted shape
// by shape, by measurement against the parent, and never in the voice variant, whose voices have each their own time
// increment and pulse shape; every other shape compiles to the code it had.  Parent / table / flag / both, kernel ms, mean
// of three interleaved runs each (profiles/plan_tables_ab.md; the parent's spread behind it):
//   four rows, SectionDelay 2 (4096 x 7500)  316.81 / 317.05 / 311.96 / 312.81  (0.46)   the flag alone
//   four rows, SectionDelay 1 (4096 x 500)   11.890 / 11.720 / 11.803 / 11.561  (0.034)  both
//   two rows, SectionDelay 2 (512 x 500)      4.800 /  4.729 /  4.765 /  4.728  (0.015)  both
//   one row, SectionDelay 1 (256 x 500)       2.428 /  2.418 /  2.422 /  2.432  (0.013)  neither: no gain
//   one row, SectionDelay 2 (256 x 500)       4.504 /  4.569 /  4.532 /  4.503  (0.010)  neither: each alone is slower
// The other float shapes (SectionDelay 3 and 4, two rows at SectionDelay 1, eight rows, the 48-lane layout) were not measured
// and take neither.
// GVTM_TUNE_PLAN_TABLES (a variant library's, for those measurements): bit 0 / bit 1 give every single-voice float shape
// the table / the flag, and no other shape either.
template <typename CT, int D, int U, int LAYOUT, bool VOICES> constexpr bool src_phase_table()
{
	constexpr bool can = sizeof(CT) == 4 && !VOICES;
	if (GVTM_TUNE_PLAN_TABLES >= 0) return can && (GVTM_TUNE_PLAN_TABLES & 1) != 0;
	return can && LAYOUT == 0 && ((U == 4 && D == 1) || (U == 2 && D == 2));
}
template <typename CT, int D, int U, int LAYOUT, bool VOICES> constexpr bool static_wavetable_pass()
{
	constexpr bool can = sizeof(CT) == 4 && !VOICES;
	if (GVTM_TUNE_PLAN_TABLES >= 0) return can && (GVTM_TUNE_PLAN_TABLES & 2) != 0;
	return can && LAYOUT == 0 && ((U == 4 && (D == 1 || D == 2)) || (U == 2 && D == 2));
}
// which float shapes run the feed-forward half of their post-tube filter stage (stage_f2) 64 steps at a time.  What a step
// of the radiation filters adds that depends on the inputs of steps n and n - 1 alone -- a x[n] - a x[n-1] -- and the sum of
// mouth, nose and throat are formed by all 64 lanes of the stage's wavefront, in place in LDS, and the two lanes of a row
// that own a recurrence keep only the recurrence.  The operations and their order are those of the serial form, so the
// bits are.  Needs the block record (float, 10 + 6 tube, not SectionDelay 3) and the owning-lanes-only serial stages; never
// the voice variant (not measured).  Adopted shape by shape, by measurement (profiles/filter_split_ab.md): parent / split,
// kernel ms, three interleaved runs each: four rows, SectionDelay 2 (4096 x 7500) 312.55 / 308.73 (-1.2 %, 3.2 times the
// parent's spread of 1.18) with 6.6 % fewer vector instructions issued -- the stage's wavefront is not what a tick waits
// for, so most of what it sheds was not time.  No other shape was timed with the split: they keep the parent's
// instruction stream (the forced library of the tests runs them bit for bit).
// GVTM_TUNE_FILTER_SPLIT (a variant library's, for those measurements): bit 0 gives every shape that can take it the
// split, and no other shape either.  (Bit 1 is kept for the pre-tube band-pass's feed-forward term, which is not built.)
template <typename CT, typename ST, int D, int U, int LAYOUT, bool VOICES> constexpr bool filter_split_f2()
{
	constexpr bool can = sizeof(CT) == 4 && sizeof(ST) == 4 && LAYOUT == 0 && D != 3 && !VOICES;
	if (GVTM_TUNE_FILTER_SPLIT >= 0) return can && (GVTM_TUNE_FILTER_SPLIT & 1) != 0;
	return can && U == 4 && D == 2;
}
template <typename CT, int D, int U, bool VOICES> constexpr bool float_arg_consts() { return sizeof(CT) == 4 && !VOICES && !far_calls_inline<D, U>(); }

template <typename CT, typename ST, int D, int U, int C, int NH, int LAYOUT_FLAGS>
__global__ __launch_bounds__((serial_waves<U, LAYOUT_FLAGS & 1>() + NH) * 64) void vtm_synth_kernel(const SynthArgs a)
{
	constexpr int LAYOUT = LAYOUT_FLAGS & 1; // gvtm_tube_layout
	constexpr bool VOICES = (LAYOUT_FLAGS & kVoicesFlag) != 0;
	constexpr bool TARGETS = (LAYOUT_FLAGS & kTargetsFlag) != 0;
	int voice = 0;
	if constexpr (VOICES) {
		voice = a.group_voice[blockIdx.x];
		if (voice < 0) return; // (uniform across the workgroup, before any barrier)
	}
	using TL = TubeLayout<LAYOUT>;
	static_assert(!TL::kWaveWide || U <= 4, "wave-wide tubes: one tube wavefront per utterance, at most four");
	constexpr int kSerial = serial_waves<U, LAYOUT>(); // serial wavefronts; the helpers follow
	static_assert(C % D == 0, "chunk must be a multiple of the section delay");
	static_assert(U == 1 || U == 2 || U == 4 || U == 8, "utterances per workgroup = DPP rows used");
	constexpr int G = (U + 3) / 4; // wavefronts per serial role
	static_assert(2 * C >= kWPre, "FIR pre-roll copy needs 2C >= kWPre");
	// internal-rate ring length: a power of two >= 2 chunks + resampler history + flush zeros, checked by the host
	// (v2_ring_length); 1024 = the reference's BUFFER_SIZE when down-sampling, which makes the ring alias exactly as
	// the reference's does in its flush overrun (see the epilogue below)
	// (several voices in a stream: each voice's ring is its single-voice stream's, whatever this launch's shape --
	// a.stream_chunk is the one-row shape's chunk, which fixes that ring)
	const int XR = VOICES ? synth_ring_for(a.kconst[voice].upsampling, a.kconst[voice].pad, a.stream ? a.stream_chunk : C) : a.xr;
	const int XRS = XR + kXMirror; // samples from one utterance's ring to the next one's (ring + mirror)
	static_assert(NH >= 1, "at least one helper wavefront");
	constexpr int kThreads = (kSerial + NH) * 64;

	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	constexpr bool kLaneRec = lane_rec<CT, LAYOUT>(); // the tube record is lane-indexed and carries the injection values
	constexpr SmemOffsets<CT, ST, U, C, kLaneRec> so;
	Smem<CT, ST, U, C> sm;
	sm.kc = reinterpret_cast<DeviceConstants*>(smem_raw + so.kc);
	sm.ext = reinterpret_cast<Extent*>(smem_raw + so.ext);
	sm.wavetable = reinterpret_cast<CT*>(smem_raw + so.wavetable);
	sm.fir = reinterpret_cast<CT*>(smem_raw + so.fir);
	sm.src = reinterpret_cast<SrcTap<ST>*>(smem_raw + so.src);
	sm.prm = reinterpret_cast<float*>(smem_raw + so.prm);
	sm.inc = reinterpret_cast<CT*>(smem_raw + so.inc);
	sm.amp = reinterpret_cast<CT*>(smem_raw + so.amp);
	sm.pos = reinterpret_cast<CT*>(smem_raw + so.pos);
	sm.noise = reinterpret_cast<CT*>(smem_raw + so.noise);
	sm.w = reinterpret_cast<CT*>(smem_raw + so.w);
	sm.usg = reinterpret_cast<CT*>(smem_raw + so.usg);
	sm.fr = reinterpret_cast<CT*>(smem_raw + so.fr);
	sm.kl = reinterpret_cast<CT*>(smem_raw + so.kl);
	sm.inj = reinterpret_cast<CT*>(smem_raw + so.inj);
	sm.lanec = reinterpret_cast<CT*>(smem_raw + so.lanec);
	sm.thy = reinterpret_cast<CT*>(smem_raw + so.thy);
	sm.ox = reinterpret_cast<CT*>(smem_raw + so.ox);
	sm.opk = reinterpret_cast<CT*>(smem_raw + so.opk);
	sm.x = reinterpret_cast<ST*>(smem_raw + so.x);
	sm.peak = reinterpret_cast<unsigned*>(smem_raw + so.peak);
	sm.dump = reinterpret_cast<CT*>(smem_raw + so.dump);
	sm.diag = reinterpret_cast<unsigned long long*>(smem_raw + so.diag);
	sm.ticket = reinterpret_cast<unsigned*>(smem_raw + so.ticket);
	sm.kb = reinterpret_cast<unsigned long long*>(smem_raw + so.kb);

	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int wave = tid >> 6;
	const int hl = lane;      // helper lane index inside its wavefront
	const size_t group = blockIdx.x;
	// GVTM_ROW_UTT(u, single-voice expression): the utterance of row u, a.batch for an empty row (see kVoicesFlag)
#define GVTM_ROW_UTT(u, ...) (VOICES ? voice_row(a, group * U + (u)) : __VA_ARGS__)
	// gvtm_stream_*: a launch continues utterances from the state an earlier launch left in device memory (a.stream)
	// and leaves its own behind.  A push synthesizes whole frames, keeps the converter's flush for later and finds the
	// frame AFTER its last one in the buffer; finish (and the one-shot entry) flushes.
	// All-float kernel, one voice: the plan constants its passes and filter wavefronts use come as floats with the kernel
	// arguments (SynthArgs::fir_k, FloatConst) -- scalar loads, off the LDS pipe this kernel keeps busy -- instead of as
	// DeviceConstants' doubles in LDS, a 64-bit read and a conversion per lane and pass.  A float plan's constants are floats
	// widened, so both are the same number.  Several voices: each workgroup's voice has its own block, in LDS.
	// The four-row shape at SectionDelay 1 keeps the LDS doubles and the library fallbacks in line: with either moved out it
	// is 3-10 % slower (DESIGN.md 6; fewer spilled registers, a worse allocation of the helper loop).
	constexpr bool kArgConsts = float_arg_consts<CT, D, U, VOICES>();
	constexpr bool kFarInline = far_calls_inline<D, U>();
#define GVTM_KF(idx, field) (kArgConsts ? static_cast<CT>(a.fir_k.f[kFirKConsts + (idx)]) : CT(k.field))
	constexpr int kFr = fr_len<CT>();
	constexpr bool kFrCompact = fr_compact<CT>();
	// start of utterance u's records in a slot
	auto at_prm = [](int slot, int u) { return rec_at<C, U>(kPrm, slot, u); };
	auto at_usg = [](int slot, int u) { return rec_at<C, U>(kF1Planes, slot, u); };
	auto at_fr = [](int slot, int u) { return rec_at<C, U>(fr_len<CT>(), slot, u); };
	// The scan, pre-tube and post-tube filter wavefronts run their stage on the lanes that own a result only (4, 36 and 8
	// of 64): measured -2.4 .. -3.2 % in float and mixed, but +7 .. +12 % with everything in double (the fp64 helper
	// passes next to them slow down by more than the stages gain), so the all-double shape keeps every lane running.
	constexpr bool kMaskedSerial = sizeof(ST) == 4;
	// Helper passes taken by position before the tickets (see the helpers' loop): one, with four utterances per workgroup on
	// the 10 + 6 tube -- float at every SectionDelay (measured with its eleven helpers: -3.8 % at SectionDelay 2, -2.4 % at 3,
	// neutral at 1 and 4; with seven helpers it had been a loss), all-double at SectionDelay 1 and 2, mixed at SectionDelay 1
	// (neutral or slower elsewhere).
	constexpr int kStaticRounds = (U == 4 && LAYOUT == 0 && (sizeof(CT) == 4 || (sizeof(ST) == 8 ? D <= 2 : D == 1))) ? 1 : 0;
	// How the helper loop says "I am a helper": through `role` or through the wavefront number.  The two are the same
	// value, but naming `role` inside the loop's closure changes what the compiler keeps in registers across it (all-double,
	// four utterances: 95 against 119 spilled registers), and neither form wins everywhere: same box, 4096 x 500 frames,
	// role / wavefront form: float SectionDelay 2 (x 2000) 97.9 / 100.3 ms, batch 256 2.43 / 2.57; fp64 SectionDelay 1
	// 25.5 / 20.4, SectionDelay 2 39.0 / 39.5, SectionDelay 3 108.8 / 112.9, 4 159.3 / 166.9; mixed SectionDelay 1 20.0 /
	// 19.1, 2 37.1 / 36.4.
	constexpr bool kHelperByRole = sizeof(CT) == 4 || D >= 3 || (sizeof(ST) == 8 && D == 2);
	constexpr bool kNoiseTable = sizeof(CT) == 4; // one-shot launches of the float model read the noise samples from the plan's table
	constexpr bool kBoundsRecurrence = bounds_by_recurrence<CT, D, U, LAYOUT>();
	constexpr bool kSrcPhaseTable = src_phase_table<CT, D, U, LAYOUT, VOICES>();
	constexpr bool kStaticWavetablePass = static_wavetable_pass<CT, D, U, LAYOUT, VOICES>();
	constexpr bool kSplitF2 = filter_split_f2<CT, ST, D, U, LAYOUT, VOICES>();
	constexpr int kKlLen = kl_len(kLaneRec);
	constexpr int kInjLen = kLaneRec ? kKlLen : kInj; // stride of a step's injection values
	auto at_kl = [](int slot, int u) { return rec_at<C, U>(kKlLen, slot, u); };
	// Lane-indexed record in BLOCKS of four steps: [block][entry][step in block].  The tube wavefront then reads an entry's
	// four steps as one 16-byte value (its own coefficient, its neighbour's, its 3-way / mouth coefficient, its injection:
	// four reads per block instead of three per step), the pre-tube filter wavefront writes its injection values once per
	// block, and a helper lane (= step) writing entry e lands on bank (20 * block + e * 4 + step) mod 32, all different
	// for the 32 lanes of a group.  (SectionDelay 3 unrolls the tube by six steps and keeps the record-per-step layout.)
	constexpr bool kBlockRec = kLaneRec && D != 3;
	auto kl_index = [](int s, int e) -> int {
		if constexpr (kBlockRec) return (s >> 2) * (kKlLen * 4) + e * 4 + (s & 3);
		else return s * kKlLen + e;
	};
	auto at_inj = [](int slot, int u) { return kLaneRec ? rec_at<C, U>(kKlLen, slot, u) + kLrInj : rec_at<C, U>(kInj, slot, u); };
	// {ax, ah1}: two planes of C per utterance (lane = step reads and writes a plane with stride 1)
	auto amp_at = [](int slot, int u, int which, int s) -> size_t {
		return ((static_cast<size_t>(slot) * U + u) * 2 + which) * C + s;
	};
	const bool kPush = a.stream_mode == kStreamPush;
	const bool kFinal = !kPush;
	using SL = StreamLayout<CT, ST>;
	constexpr int kTubeLanes = TubeLayout<LAYOUT>::kLanes;
	constexpr int kTubeWords = 2 * D + 1;

	// ---- constants, extents and design tables into LDS; clear rings and pre-rolls
	{
		const int* src = reinterpret_cast<const int*>(VOICES ? a.kconst + voice : a.kconst);
		int* dst = reinterpret_cast<int*>(sm.kc);
		for (int i = tid; i < static_cast<int>(sizeof(DeviceConstants) / sizeof(int)); i += kThreads) dst[i] = src[i];
	}
	// design tables: fp64 in device memory, or float as designed by the host when everything runs in float
	for (int i = tid; i < kWavetableLength; i += kThreads) sm.wavetable[i] = VOICES ? static_cast<const CT*>(a.wavetable)[static_cast<size_t>(voice) * kWavetableLength + i] : static_cast<const CT*>(a.wavetable)[i];
	for (int i = tid; i < kSrcFilterLength; i += kThreads) {
		if constexpr (kSrcHOnly<CT, ST, U>) {
			reinterpret_cast<ST*>(sm.src)[i] = static_cast<ST>(static_cast<const CT*>(a.src_h)[i]);
			if (i == 0) reinterpret_cast<ST*>(sm.src)[kSrcFilterLength] = ST(0); // deltaH_[last] = 0 - h_[last] (SampleRateConverter.h:254)
		} else {
			sm.src[i].h = static_cast<ST>(static_cast<const CT*>(a.src_h)[i]);
			sm.src[i].dh = static_cast<ST>(static_cast<const CT*>(a.src_dh)[i]);
		}
	}
	for (int i = tid; i < 3 * U * (kWPre + 2 * C); i += kThreads) sm.w[i] = CT(0.0);
	for (int i = tid; i < U * XRS; i += kThreads) sm.x[i] = ST(0);
	__syncthreads();
	if (tid < U) {
		Extent e{0, 0, 0, 0, 0ull, 0ull};
		const size_t ug = GVTM_ROW_UTT(tid, group * U + tid);
		unsigned peak0 = 0u;
		if (ug < a.batch) {
			// a stream's push carries one more row than it synthesizes: the next frame, which the last one interpolates towards
			// (not from targets: a step does not interpolate towards a successor)
			const size_t rows_avail = a.max_frames - (kPush && !TARGETS ? 1 : 0);
			const int f = a.frame_counts ? a.frame_counts[ug] : static_cast<int>(rows_avail);
			// device-resident counts cannot be validated by the host: clamp to the allocated frames
			e.frames = f > 0 ? (static_cast<size_t>(f) < rows_avail ? f : static_cast<int>(rows_avail)) : 0;
			// (targets: the counts are steps, and `frames` holds them)
			e.steps = TARGETS ? static_cast<uint32_t>(e.frames) : static_cast<uint32_t>(e.frames) * sm.kc->control_steps;
			e.nchunks = e.steps == 0 ? 1 : static_cast<int>((e.steps + C - 1) / C);
			e.last_frame = e.frames - 1 + (kPush ? 1 : 0);
			if (a.stream) {
				const StreamHeader* h = reinterpret_cast<const StreamHeader*>(a.stream + ug * a.stream_stride);
				e.step_base = h->step_base;
				e.k_first = ((e.step_base << 16) + sm.kc->time_inc - 1) / sm.kc->time_inc;
				peak0 = h->peak_bits;
			}
		}
		sm.ext[tid] = e;
		sm.peak[tid] = peak0;
	}
	if (tid < 8) sm.diag[tid] = 0ull;
	if (tid < 65) {
		// per-lane fixed junction coefficient of the tube layout (0, -1 for the tube input, or a fixed
		// nasal coefficient); slot 64 is the zero that lanes without injection read
		const LaneSpec sp = TL::lane(TL::kWaveWide ? tid : (tid & 15));
		CT v = CT(0.0);
		if (tid < 64 && sp.kl_slot < 0 && tid < (TL::kWaveWide ? TL::kLanes : 64)) {
			v = sp.kl_fixed == 1 ? -CT(1.0) : (sp.kl_fixed >= 2 ? CT(sm.kc->nasal_k[sp.kl_fixed - 1]) : CT(0.0));
		}
		sm.lanec[tid] = v;
		if (tid < 64) {
			const LaneSpec ps = TL::lane(TL::kWaveWide ? tid : (tid & 15));
			reinterpret_cast<int*>(sm.lanec + 72)[tid] = (ps.link_right & 7) | ((ps.kl_slot + 1) << 4) | (ps.kl_fixed << 8) | (ps.damp_left << 12) | ((ps.inj_slot + 1) << 16);
		}
	}
	if constexpr (kLaneRec) {
		// the entries of the lane-indexed tube record that never change, in every record of both slots
		for (int i = tid; i < 2 * U * C; i += kThreads) {
			const int slot = i / (U * C), r = i - slot * (U * C), u = r / C, sstep = r - u * C;
			CT* kr = sm.kl + at_kl(slot, u);
#pragma unroll
			for (int Lq = 0; Lq < 16; ++Lq) {
				const LaneSpec sp = TL::lane(Lq);
				if (sp.kl_slot < 0) kr[kl_index(sstep, Lq)] = sp.kl_fixed == 1 ? -CT(1.0) : (sp.kl_fixed >= 2 ? CT(sm.kc->nasal_k[sp.kl_fixed - 1]) : CT(0.0));
			}
			kr[kl_index(sstep, kLrZero)] = CT(0.0);
			kr[kl_index(sstep, kLrKn)] = CT(sm.kc->nasal_k[5]); // nose aperture coefficient (fixed)
		}
	}
	if constexpr (kHelperByRole || kStaticRounds > 0) {
		if (tid < 4) sm.ticket[tid] = tid < 2 ? static_cast<unsigned>(kStaticRounds * NH) : 0u;
	} else {
		if (tid < 4) sm.ticket[tid] = 0u;
	}
	if constexpr (kBoundsRecurrence) {
		if (tid == 0) {
			const SrcBoundsStep bstep = src_bounds_step(sm.kc->time_inc, C);
			sm.ticket[2] = bstep.dq;
			sm.ticket[3] = bstep.dr;
		}
	}
	for (int i = tid; i < kMaxFirTaps; i += kThreads) sm.fir[i] = i < sm.kc->fir_taps ? static_cast<const CT*>(a.fir)[i] : CT(0.0);
	__syncthreads();

	if (a.stream) {
		// the resampler's ring, the decimator's pre-roll (the 48 oversampled source values in front of the next step)
		for (int u = 0; u < U; ++u) {
			if (GVTM_ROW_UTT(u, group * U + u) >= a.batch) break;
			const unsigned char* sb = a.stream + GVTM_ROW_UTT(u, (group * U + u)) * a.stream_stride;
			const ST* ring = reinterpret_cast<const ST*>(sb + SL::ring(kTubeLanes, kTubeWords));
			for (int i = tid; i < XRS; i += kThreads) sm.x[u * XRS + i] = ring[i < XR ? i : i - XR];
			const CT* pre = reinterpret_cast<const CT*>(sb + SL::wpre(kTubeLanes, kTubeWords));
			for (int i = tid; i < kWPre; i += kThreads) sm.w[static_cast<size_t>(u) * (kWPre + 2 * C) + i] = pre[i];
		}
		__syncthreads();
	}

	const DeviceConstants& k = *sm.kc;
	int max_chunks = 0;
#pragma unroll
	for (int u = 0; u < U; ++u) max_chunks = sm.ext[u].nchunks > max_chunks ? sm.ext[u].nchunks : max_chunks;

	// steps of utterance u inside chunk c: -1 = the chunk does not exist for it
	auto valid_in = [&](int u, int c) -> int {
		const Extent e = sm.ext[u];
		if (c < 0 || c >= e.nchunks) return -1;
		const uint32_t left = e.steps - static_cast<uint32_t>(c) * C;
		return left < static_cast<uint32_t>(C) ? static_cast<int>(left) : C;
	};

	// ---- persistent role state (each wavefront only ever touches its own role's variables)
	// section lane inside the tube / filter wavefronts: a 16-lane DPP row per utterance, or the whole
	// wavefront for the 48-section tube
	// (a wave-wide tube with several utterances per workgroup: the tube wavefronts use the whole wavefront, the
	// other serial roles the row view)
	constexpr bool kRowView = !TL::kWaveWide || U > 1;
	const int L = kRowView ? (lane & 15) : lane;
	const int row = kRowView ? (lane >> 4) : 0;
	// serial wavefronts: role = wave / G (tube, scan, pre-tube filters, post-tube filters, interpolation),
	// sub = wave % G picks the group of four utterances; helpers follow
	constexpr bool kTubePerWave = TL::kWaveWide && U > 1; // U tube wavefronts, one wavefront per other serial role
	constexpr int kFirstHelper = kTubePerWave ? kSerial : 5 * G;
	const int role = kTubePerWave ? (wave < U ? 0 : (wave < kSerial ? wave - U + 1 : 5)) : (wave < 5 * G ? wave / G : 5);
	const int sub = kTubePerWave ? (wave < U ? wave : 0) : (wave < 5 * G ? wave % G : 0);
	const int urow = (U >= 4) ? sub * 4 + row : row % U; // utterance served by this DPP row (rows beyond U mirror)
	// A wavefront runs ONE serial role for the whole kernel, so the recurrence states of the
	// roles share one small register array instead of each occupying registers in every wave.
	constexpr int kState = (2 * D + 1) > 5 ? (2 * D + 1) : 5;
	CT st[kState];
#pragma unroll
	for (int i = 0; i < kState; ++i) st[i] = CT(0.0);
	// S: oscillator position, noise seed (NoiseSource.h:32-34), previous white sample
	CT& sc_pos = st[0];
	CT& sc_prev = st[2];
	double sc_seed = 0.7892347; // NoiseSource is double whatever TFloat is (NoiseSource.h:52-54)
	// T: top/bottom delay lines of my section (D deep), reflection-filter state of the end lanes
	CT* const top = st;
	CT* const bot = st + D;
	CT& refl_y1 = st[2 * D];
	// F1: band-pass and throat filter states;  F2: radiation filter state
	CT& bp_x1 = st[0];
	CT& bp_x2 = st[1];
	CT& bp_y1 = st[2];
	CT& bp_y2 = st[3];
	CT& thr_y1 = st[4];
	CT& rad_x1 = st[0];
	CT& rad_y1 = st[1];
	// I: lane L of row u interpolates parameter L of utterance u
	float ip_cur = 0.f, ip_delta = 0.f, ip_this = 0.f, ip_next = 0.f, ip_next2 = 0.f;
	uint32_t ip_j = 0;
	int ip_frame = 0;
	const int Lp = lane & 15;  // parameter index of an interpolation lane
	const int rowp = sub * 4 + (lane >> 4); // its utterance
	if (!TARGETS && role == 4 && rowp < U) {
		const int frames = sm.ext[rowp].frames;
		const int last = sm.ext[rowp].last_frame;
		if (frames > 0) {
			const float* __restrict__ P = a.params + GVTM_ROW_UTT(rowp, (group * U + rowp)) * a.max_frames * 16;
			ip_this = P[Lp];
			ip_next = P[static_cast<size_t>(last > 1 ? 1 : last) * 16 + Lp];
			ip_next2 = P[static_cast<size_t>(last > 2 ? 2 : last) * 16 + Lp];
		}
	}
	// I, from targets: lane L of row u walks the points of utterance u's list for parameter L (vtm_targets.hpp): the filter's
	// sum, the entering and the leaving value, the two cursors and the steps at which they move next.  (A refused utterance
	// has 0 steps: its list ids and offsets are never read.)
	// A stream's launch walks absolute steps from the utterance's step_base on: behind step 0 the walk resumes on the sum the
	// previous launch left in the stream state (targets_resume; the points are the stream's log, in absolute steps), and the
	// epilogue stores the sum back.  An utterance the launch does not advance keeps its sums.
	[[maybe_unused]] TargetsWalk tg{};
	[[maybe_unused]] int64_t tg_base = 0;
	// Several voices: the filter's length and its reciprocal are the workgroup's voice's, one uniform read each from the plan's
	// per-voice tables, here and never per step; with one voice the arguments themselves serve.
	[[maybe_unused]] int64_t tgv_N = 0;
	[[maybe_unused]] double tgv_invN = 0.0;
	if constexpr (TARGETS && VOICES) {
		tgv_N = a.tg_voice_N[voice];
		tgv_invN = a.tg_voice_invN[voice];
	}
	if constexpr (TARGETS) {
		// (an empty row of a launch of several voices has 0 frames, as a refused utterance has: it begins no walk)
		if (role == 4 && rowp < U && sm.ext[rowp].frames > 0) {
			const size_t slot = GVTM_ROW_UTT(rowp, (group * U + rowp)) * GVTM_N_PARAM + Lp;
			const int64_t list = a.tg_ids ? static_cast<int64_t>(a.tg_ids[slot]) : static_cast<int64_t>(slot);
			if (a.stream) tg_base = static_cast<int64_t>(sm.ext[rowp].step_base);
			if (tg_base > 0) {
				const double* sums = reinterpret_cast<const double*>(a.stream + GVTM_ROW_UTT(rowp, (group * U + rowp)) * a.stream_stride + SL::sums(kTubeLanes, kTubeWords, XR));
				targets_resume(tg, a.tg_steps, a.tg_values, a.tg_offsets[list], a.tg_offsets[list + 1], VOICES ? tgv_N : a.tg_N, tg_base, sums[Lp]);
			} else {
				targets_begin(tg, a.tg_steps, a.tg_values, a.tg_offsets[list], a.tg_offsets[list + 1], VOICES ? tgv_N : a.tg_N);
			}
		}
	}

	// first helper wavefront, lanes 0 .. U (stage_bounds): quotient and remainder of src_bounds_advance (csrc/vtm_design.hpp)
	// at the chunk boundary the lane reports next.  Lane 0 starts at utterance 0's step_base, where the quotient is k_first
	// (one multiplication gives its remainder); lane 1 + u one chunk behind utterance u's.
	[[maybe_unused]] SrcBounds bnd{0ull, 0u};
	if constexpr (kBoundsRecurrence) {
		if (wave == kFirstHelper && lane <= U) {
			const Extent e = sm.ext[lane == 0 ? 0 : lane - 1];
			bnd.q = e.k_first;
			bnd.r = static_cast<unsigned>((e.step_base << 16) + k.time_inc - 1 - e.k_first * k.time_inc);
			if (lane > 0) src_bounds_advance(bnd, SrcBoundsStep{sm.ticket[2], sm.ticket[3]}, k.time_inc);
		}
	}

	// a stream's recurrence states as the previous launch left them (all zero and the fresh noise seed after create / reset)
	const int tube_utt = kTubePerWave ? sub : urow;           // utterance of a tube lane
	const int serial_utt = (role == 0) ? tube_utt : urow;      // utterance of a lane of any serial wavefront
	const bool serial_live = role < 4 && serial_utt < U && GVTM_ROW_UTT(serial_utt, group * U + serial_utt) < a.batch;
	if (a.stream && serial_live) {
		const unsigned char* sb = a.stream + GVTM_ROW_UTT(serial_utt, (group * U + serial_utt)) * a.stream_stride;
		const CT* sc = reinterpret_cast<const CT*>(sb + SL::scalars());
		if (role == 1) {
			sc_pos = sc[kSsPos];
			sc_prev = sc[kSsPrev];
			sc_seed = reinterpret_cast<const StreamHeader*>(sb)->seed;
		} else if (role == 2) {
			bp_x1 = sc[kSsBp]; bp_x2 = sc[kSsBp + 1]; bp_y1 = sc[kSsBp + 2]; bp_y2 = sc[kSsBp + 3];
			thr_y1 = sc[kSsThr];
		} else if (role == 3) {
			const int w2 = (L == 0) ? kSsRadMouth : kSsRadNose;
			rad_x1 = sc[w2];
			rad_y1 = sc[w2 + 1];
		} else if (role == 0) {
			const int Lt = kTubePerWave ? lane : L;
			if (Lt < kTubeLanes) {
				const CT* tb = reinterpret_cast<const CT*>(sb + SL::tube()) + Lt * kTubeWords;
#pragma unroll
				for (int i = 0; i < kTubeWords; ++i) st[i] = tb[i];
			}
		}
	}

	unsigned long long role_busy = 0;
#if GVTM_TUNE_TRACE
	// diagnostics variant: workgroup 0 leaves a timeline of two ticks behind the per-group counters
	int tr_n = 0;
	auto TR = [&](int t, unsigned id) {
		if (a.phase_cycles != nullptr && group == 0 && lane == 0 && t >= GVTM_TUNE_TRACE && t < GVTM_TUNE_TRACE + 2 && tr_n < 128)
			a.phase_cycles[32768 + wave * 128 + tr_n++] = (static_cast<unsigned long long>(id) << 48) | (clock64() & 0xFFFFFFFFFFFFull);
	};
#else
	auto TR = [](int, unsigned) {};
#endif
	const bool stamping = a.phase_cycles != nullptr && lane == 0;

	// -------------------------------------------------------------------------------------
	// helper stages

	// P2a: pitch / glottal volume / aspiration volume -> phase increment, ax, ah1
	auto stage_p2a = [&](int c, int pass) {
		for (int item = pass * 64 + hl; item < U * C && item < (pass + 1) * 64; item += 64) {
			const int u = item / C, s = item - u * C;
			if (s >= valid_in(u, c)) continue;
			const float* pv = sm.prm + at_prm(c & 1, u) + s * kPrm;
			const CT pitch = pv[0], gv = pv[1], av = pv[2];
			// Util::frequency (VTMUtil.h:74-84) -> oscillator increment (WavetableGlottalSource.h:198, :218)
			const CT f0 = frequency_dev<kFarInline>(pitch);
			sm.inc[((c & 1) * U + u) * C + s] = (f0 / CT(2.0)) * GVTM_KF(kKfBasicIncrement, basic_increment);
			sm.amp[amp_at(c & 3, u, 0, s)] = amplitude_60db_dev<kFarInline>(gv);
			sm.amp[amp_at(c & 3, u, 1, s)] = amplitude_60db_dev<kFarInline>(av);
		}
	};

	// P4a: wavetable lookup + linear interpolation at the 2x oversampled rate
	// P4a: the wavetable oscillator's two lookups per step (WavetableGlottalSource.h:212-235), one item per half step.
	// A pass takes kP4aItems items per lane, the reads of all of them side by side: position -> table entries -> store
	// is three dependent LDS round trips of several hundred cycles each under load, for some 25 instructions.
	constexpr int kP4aItems = 1; // (two per lane: pass time 170 -> 123 cycles per step but the kernel no faster -- fewer, longer passes at a tick's end)
	auto stage_p4a = [&](int c, int pass) {
		if constexpr (kStaticWavetablePass) {
			// The plan has said that the table never follows the amplitude (a.static_wavetable; every shipped voice): position,
			// the two entries, interpolate, store -- no amplitude read and nothing from the constants block, which
			// wavetable_entry below reads (waveform, tn_delta, the two divisions) and waits for before its first table read.
			if (a.static_wavetable != 0) {
				static_assert(kP4aItems == 1, "one item per lane and pass");
				const int item = pass * 64 + hl;
				const int u = item / (2 * C), h = item - u * 2 * C;
				if (item >= U * 2 * C || h >= 2 * valid_in(u, c)) return;
				const CT p = sm.pos[((c & 1) * U + u) * 2 * C + h];
				// a position in (-1, 0) truncates towards zero, as the reference's cast does
				const unsigned lower = static_cast<unsigned>(static_cast<int>(p));
				const unsigned upper = (lower + 1 > 511u) ? lower + 1 - 512u : lower + 1;
				const CT wl = sm.wavetable[lower];
				const CT wu = sm.wavetable[upper];
				const CT v = wl + rmul(p - static_cast<CT>(lower), wu - wl);
				CT* slot = sm.w + (static_cast<size_t>(c % 3) * U + u) * (kWPre + 2 * C);
				slot[kWPre + h] = v;
				if (GVTM_KERNEL_TAPS && a.debug_taps) {
					a.debug_taps[(GVTM_ROW_UTT(u, (group * U + u)) * a.max_frames * k.control_steps + static_cast<size_t>(c) * C + (h >> 1)) * 8 + 5 + (h & 1)] = p;
				}
				if (h >= 2 * C - kWPre) {
					// the tail of a chunk doubles as the FIR pre-roll of the next one
					CT* next = sm.w + (static_cast<size_t>((c + 1) % 3) * U + u) * (kWPre + 2 * C);
					next[h - (2 * C - kWPre)] = v;
				}
				return;
			}
		}
		if constexpr (U == 1) {
			// one item per lane, reads where they are needed (one utterance per workgroup: measured 1-3 % faster this way)
			for (int item = pass * 64 + hl; item < U * 2 * C && item < (pass + 1) * 64; item += 64) {
				const int u = item / (2 * C), h = item - u * 2 * C;
				if (h >= 2 * valid_in(u, c)) continue;
				const CT p = sm.pos[((c & 1) * U + u) * 2 * C + h];
				const unsigned lower = static_cast<unsigned>(static_cast<int>(p));
				const unsigned upper = (lower + 1 > 511u) ? lower + 1 - 512u : lower + 1;
				const CT ax = sm.amp[amp_at(c & 3, u, 0, h >> 1)];
				const CT wl = wavetable_entry(sm.wavetable, k, lower, ax);
				const CT wu = wavetable_entry(sm.wavetable, k, upper, ax);
				const CT v = wl + rmul(p - static_cast<CT>(lower), wu - wl);
				CT* slot = sm.w + (static_cast<size_t>(c % 3) * U + u) * (kWPre + 2 * C);
				slot[kWPre + h] = v;
				if (GVTM_KERNEL_TAPS && a.debug_taps) {
					a.debug_taps[(GVTM_ROW_UTT(u, (group * U + u)) * a.max_frames * k.control_steps + static_cast<size_t>(c) * C + (h >> 1)) * 8 + 5 + (h & 1)] = p;
				}
				if (h >= 2 * C - kWPre) {
					CT* next = sm.w + (static_cast<size_t>((c + 1) % 3) * U + u) * (kWPre + 2 * C);
					next[h - (2 * C - kWPre)] = v;
				}
			}
			return;
		}
		int item[kP4aItems], u[kP4aItems], h[kP4aItems];
		bool on[kP4aItems];
		CT p[kP4aItems], ax[kP4aItems];
#pragma unroll
		for (int q = 0; q < kP4aItems; ++q) {
			item[q] = (pass * kP4aItems + q) * 64 + hl;
			u[q] = item[q] / (2 * C);
			h[q] = item[q] - u[q] * 2 * C;
			on[q] = item[q] < U * 2 * C && h[q] < 2 * valid_in(u[q] < U ? u[q] : 0, c);
			if (!on[q]) { u[q] = 0; h[q] = 0; }
			p[q] = sm.pos[((c & 1) * U + u[q]) * 2 * C + h[q]];
			ax[q] = sm.amp[amp_at(c & 3, u[q], 0, h[q] >> 1)];
		}
		asm volatile("" ::: "memory");
#pragma unroll
		for (int q = 0; q < kP4aItems; ++q) p[q] = on[q] ? p[q] : CT(0.0); // (an item that does not exist reads entry 0)
		unsigned lower[kP4aItems];
		CT wl[kP4aItems], wu[kP4aItems];
#pragma unroll
		for (int q = 0; q < kP4aItems; ++q) {
			// a position in (-1, 0) truncates towards zero, as the reference's cast does
			lower[q] = static_cast<unsigned>(static_cast<int>(p[q]));
			const unsigned upper = (lower[q] + 1 > 511u) ? lower[q] + 1 - 512u : lower[q] + 1;
			wl[q] = wavetable_entry(sm.wavetable, k, lower[q], ax[q]);
			wu[q] = wavetable_entry(sm.wavetable, k, upper, ax[q]);
		}
		asm volatile("" ::: "memory");
#pragma unroll
		for (int q = 0; q < kP4aItems; ++q) {
			if (!on[q]) continue;
			const CT v = wl[q] + rmul(p[q] - static_cast<CT>(lower[q]), wu[q] - wl[q]);
			CT* slot = sm.w + (static_cast<size_t>(c % 3) * U + u[q]) * (kWPre + 2 * C);
			slot[kWPre + h[q]] = v;
			if (GVTM_KERNEL_TAPS && a.debug_taps) {
				a.debug_taps[(GVTM_ROW_UTT(u[q], (group * U + u[q])) * a.max_frames * k.control_steps + static_cast<size_t>(c) * C + (h[q] >> 1)) * 8 + 5 + (h[q] & 1)] = p[q];
			}
			if (h[q] >= 2 * C - kWPre) {
				// the tail of a chunk doubles as the FIR pre-roll of the next one
				CT* next = sm.w + (static_cast<size_t>((c + 1) % 3) * U + u[q]) * (kWPre + 2 * C);
				next[h[q] - (2 * C - kWPre)] = v;
			}
		}
	};

	// P4b: 2:1 FIR decimator (WavetableGlottalSourceFIRFilter.h:276-304) and the source mix of
	// execSynthesisStep (VocalTractModel0.h:416-438)
	auto stage_p4b = [&](int c, int pass) {
		const int taps = k.fir_taps;
		for (int item = pass * 64 + hl; item < U * C && item < (pass + 1) * 64; item += 64) {
			const int u = item / C, s = item - u * C;
			if (s >= valid_in(u, c)) continue;
			// (the noise sample of a one-shot launch comes from the plan's table: requested first, used after the taps)
			CT lp_table = CT(0.0);
			if (kNoiseTable && a.noise_lp != nullptr) lp_table = static_cast<const CT*>(a.noise_lp)[sm.ext[u].step_base + static_cast<unsigned long long>(c) * C + s];
			const CT* wp = sm.w + (static_cast<size_t>(c % 3) * U + u) * (kWPre + 2 * C) + kWPre + 2 * s + 1;
			// acc = sum_i w[n - i] * c[i] in tap order (WavetableGlottalSourceFIRFilter.h:285-288); samples
			// and coefficients are fetched as aligned pairs (n is odd, so w[n-i-1], w[n-i] pair up for even i)
			using CT2 = typename Pair<CT>::type;
			CT acc = 0;
			// float: each product rounded, as the reference's decimator does (the FIR output feeds the tube, whose
			// resonances magnify a fused-MAC difference); double: one fused operation per tap, spelled out
			auto fir_mad = [](CT w, CT cf, CT sum) -> CT {
				if constexpr (sizeof(CT) == 4) return sum + rmul(w, cf);
				else return __builtin_fma(w, cf, sum);
			};
			// The design always yields 49 taps in double and 47 in float (WavetableGlottalSourceFIRFilter.h:137-235 with the
			// constants of WavetableGlottalSource.h:94-96): the float tap loop is unrolled over that count, so that the 24
			// paired LDS reads of a lane are all in flight together instead of one round trip per pair, and its coefficients
			// are the 32-bit literals of kGlottalFirF32 (vtm_design.hpp) -- the same 47 floats for every voice, rate and plan,
			// so they need no register, no load and no reload (as kernel arguments they were 47 SGPRs that spilled, and
			// the block reloaded 37 of them lane by lane on the vector pipe).  a.fir_literals: the host found its own design
			// equal to the table bit for bit; otherwise, and in double, the generic loop over the plan's coefficients in LDS.
			// (The two shapes fir_literal_taps() leaves out keep the plan's own 47 coefficients in SGPRs, a.fir_k.f, under the
			// condition they always had: right for any design of that length, so they have nothing to ask the flag.)
			// (float only: a double is no literal, and 98 coefficient SGPRs with the reads in flight cost more registers than
			// the workgroup has to spare: measured 6-8 % slower at batch 4096)
			constexpr int kNT = kGlottalFirTapsF32;
			constexpr bool kLiteralTaps = fir_literal_taps<D, U>();
			if (sizeof(CT) == 4 && (kLiteralTaps ? a.fir_literals != 0 : taps == kNT)) {
				// every read first (the compiler, left alone, issues them two at a time between the multiply-adds and waits
				// for each pair: a dozen LDS round trips in a row made this the longest per-step pass), then the arithmetic
				CT2 wv[kNT / 2];
#pragma unroll
				for (int i = 0; i + 1 < kNT; i += 2) wv[i / 2] = *reinterpret_cast<const CT2*>(wp - i - 1);
				const CT wlast = wp[-(kNT - 1)];
				asm volatile("" ::: "memory");
#pragma unroll
				for (int i = 0; i + 1 < kNT; i += 2) {
					acc = fir_mad(wv[i / 2].y, CT(kLiteralTaps ? kGlottalFirF32[i] : a.fir_k.f[i]), acc);
					acc = fir_mad(wv[i / 2].x, CT(kLiteralTaps ? kGlottalFirF32[i + 1] : a.fir_k.f[i + 1]), acc);
				}
				acc = fir_mad(wlast, CT(kLiteralTaps ? kGlottalFirF32[kNT - 1] : a.fir_k.f[kNT - 1]), acc);
			} else {
				int i = 0;
				if constexpr (U >= 4) {
				// (four utterances per workgroup only: with one or two the tube is the tick and these measured 1-5 % slower)
				// groups of four sample / coefficient pairs, all eight reads before the eight multiply-adds (taken pair by
				// pair every pair waited for its own LDS round trip: 25 in a row for the 49 taps of the double models)
				for (; i + 7 < taps; i += 8) {
					CT2 wv[4], cv[4];
#pragma unroll
					for (int g = 0; g < 4; ++g) {
						wv[g] = *reinterpret_cast<const CT2*>(wp - i - 2 * g - 1);
						cv[g] = *reinterpret_cast<const CT2*>(sm.fir + i + 2 * g);
					}
					asm volatile("" ::: "memory");
#pragma unroll
					for (int g = 0; g < 4; ++g) {
						acc = fir_mad(wv[g].y, cv[g].x, acc);
						acc = fir_mad(wv[g].x, cv[g].y, acc);
					}
				}
				}
				for (; i + 1 < taps; i += 2) {
					const CT2 wv = *reinterpret_cast<const CT2*>(wp - i - 1);
					const CT2 cv = *reinterpret_cast<const CT2*>(sm.fir + i);
					acc = fir_mad(wv.y, cv.x, acc);
					acc = fir_mad(wv.x, cv.y, acc);
				}
				if (i < taps) acc = fir_mad(wp[-i], sm.fir[i], acc);
			}
			const CT ax = sm.amp[amp_at(c & 3, u, 0, s)], ah1 = sm.amp[amp_at(c & 3, u, 1, s)];
			const CT lp = (kNoiseTable && a.noise_lp != nullptr) ? lp_table : sm.noise[((c % 3) * U + u) * C + s];
			CT pulse = acc;
			const CT pulsed_noise = rmul(lp, pulse);
			pulse = rmul(ax, rmul(pulse, CT(1.0) - GVTM_KF(kKfBreathiness, breathiness)) + rmul(pulsed_noise, GVTM_KF(kKfBreathiness, breathiness)));
			CT signal;
			if (k.modulation) {
				CT cm = rmul(ax, GVTM_KF(kKfCrossmix, crossmix_factor));
				cm = cm < CT(1.0) ? cm : CT(1.0);
				signal = rmul(pulsed_noise, cm) + rmul(lp, CT(1.0) - cm);
			} else {
				signal = lp;
			}
			CT* usg = sm.usg + at_usg(c & 1, u) + s;
			const CT tube_in = (pulse + rmul(ah1, signal)) * CT(0.125), throat_in = pulse * CT(0.125);
			usg[kF1U * C] = tube_in;
			usg[kF1Sig * C] = signal;
			usg[kF1Thr * C] = throat_in;
			if (GVTM_KERNEL_TAPS && a.debug_taps) {
				double* t = a.debug_taps + (GVTM_ROW_UTT(u, (group * U + u)) * a.max_frames * k.control_steps + static_cast<size_t>(c) * C + s) * 8;
				t[0] = tube_in; t[1] = signal; t[2] = throat_in; t[3] = acc; t[4] = lp;
			}
		}
	};

	// P2c: frication volume / position / centre frequency / bandwidth -> taps, band-pass design
	auto stage_p2c = [&](int c, int pass) {
		for (int item = pass * 64 + hl; item < U * C && item < (pass + 1) * 64; item += 64) {
			const int u = item / C, s = item - u * C;
			if (s >= valid_in(u, c)) continue;
			const float* pv = sm.prm + at_prm(c & 1, u) + s * kPrm;
			const CT fvol = pv[3], fpos = pv[4], fcf = pv[5], fbw = pv[6];
			CT* fr = sm.fr + at_fr(c & 1, u) + s * kFr;
			// setFricationTaps (VocalTractModel0.h:524-552)
			const CT amp = amplitude_60db_dev<kFarInline>(fvol);
			const int ipart = static_cast<int>(fpos);
			const CT complement = fpos - ipart;
			const CT remainder = CT(1.0) - complement;
			// taps[ipart] = remainder * amp, taps[ipart + 1] = complement * amp, the others 0 (a share that would go to a
			// ninth section is dropped): the pre-tube filter wavefront hands each section its share.  The reference writes
			// the second share only from inside the i == ipart branch of its loop over sections 0..7, so for ipart == -1
			// (a position in (-2, -1)) section 0 gets nothing either.
			if constexpr (kFrCompact) {
				fr[kFrTapA] = remainder * amp;
				fr[kFrTapB] = complement * amp;
				fr[kFrZero] = CT(0.0);
				*reinterpret_cast<int*>(fr + kFrFirst) = ipart == -1 ? 8 : ipart; // (8: every section's distance is out of 0..1)
			} else {
#pragma unroll
				for (int q = 0; q < 8; ++q) {
					CT t = CT(0.0);
					if (q == ipart) t = remainder * amp;
					else if (q >= 1 && q == ipart + 1) t = complement * amp;
					fr[q] = t;
				}
				fr[kFr - 1] = CT(0.0); // the zero tap read by sections without frication injection
			}
			// BandpassFilter::update (BandpassFilter.h:91-110)
			const CT pi = CT(3.14159265358979323846);
			const CT tan_v = tan_dev<kFarInline>(pi * fbw * GVTM_KF(kKfBpT, bp_T));
			const CT cos_v = cos_dev<kFarInline>(CT(2.0) * pi * fcf * GVTM_KF(kKfBpT, bp_T));
			const CT a2 = (CT(1.0) - tan_v) / (CT(1.0) + tan_v);
			CT* bpc = sm.usg + at_usg(c & 1, u) + s;
			bpc[kF1B0 * C] = CT(0.5) - rmul(CT(0.5), a2);
			bpc[kF1A1 * C] = -(CT(1.0) + a2) * cos_v;
			bpc[kF1A2 * C] = a2;
		}
	};

	// P2b: radii and velum -> junction coefficients as the tube lanes consume them
	auto stage_p2b = [&](int c, int pass) {
		for (int item = pass * 64 + hl; item < U * C && item < (pass + 1) * 64; item += 64) {
			const int u = item / C, s = item - u * C;
			if (s >= valid_in(u, c)) continue;
			const float* cur = sm.prm + at_prm(c & 1, u) + s * kPrm + 7;
			// setAllParameters (VocalTractModel0.h:698-716): radius scaling and floor
			CT r2[8];
#pragma unroll
			for (int q = 0; q < 8; ++q) {
				CT r = static_cast<CT>(cur[q]) * GVTM_KF(kKfRadiusCoef + q, radius_coef[q]);
				r = r > CT(0.01) ? r : CT(0.01);
				r2[q] = rmul(r, r);
			}
			const CT velum2 = rmul(static_cast<CT>(cur[8]), static_cast<CT>(cur[8]));
			// calculateTubeCoefficients (VocalTractModel0.h:484-512)
			CT kj[8];
#pragma unroll
			// (fdiv_n: the division without range scaling -- squared radii are >= 1e-4 and of moderate size)
			for (int q = 0; q < 7; ++q) kj[q] = fdiv_n(r2[q] - r2[q + 1], r2[q] + r2[q + 1]);
			kj[7] = fdiv_n(r2[7] - GVTM_KF(kKfAperture2, aperture_radius2), r2[7] + GVTM_KF(kKfAperture2, aperture_radius2));
			const CT asum = fdiv_n(CT(2.0), r2[3] + r2[3] + velum2);
			const CT nk1 = fdiv_n(velum2 - GVTM_KF(kKfNasalR2Sq, nasal_r2_sq), velum2 + GVTM_KF(kKfNasalR2Sq, nasal_r2_sq));
			// compact record: the tube lanes pick their slot through the layout table
			CT* kl = sm.kl + at_kl(c & 1, u) + (kLaneRec ? 0 : s * kKlLen);
			if constexpr (kLaneRec) {
				// lane-indexed record: every section lane's left coefficient at its lane index
#pragma unroll
				for (int Lq = 0; Lq < 16; ++Lq) {
					const int q = TL::lane(Lq).kl_slot;
					if (q >= 0) kl[kl_index(s, Lq)] = (q == kKlNk1) ? nk1 : kj[q < 7 ? q : 0];
				}
				kl[kl_index(s, kLrAlr)] = asum * r2[3];
				kl[kl_index(s, kLrAu)] = asum * velum2;
				kl[kl_index(s, kLrK8)] = kj[7];
				sm.opk[((c % 3) * U + u) * C + s] = CT(1.0) + kj[7]; // the radiated part is (1 + k) * top (F2 multiplies)
			} else {
#pragma unroll
				for (int q = 0; q < 7; ++q) kl[q] = kj[q]; // J1..J7
				kl[kKlK8] = kj[7];                         // J8: last section | air
				kl[kKlNk1] = nk1;                          // NJ1: velum | first fixed nasal radius
				kl[kKlAlr] = asum * r2[3];
				kl[kKlAu] = asum * velum2;
			}
		}
	};

	// output samples [.., v) are available; what of them the aligned grid lets a non-final chunk emit
	auto grid_floor = [](unsigned long long v, unsigned long long k_first) -> unsigned long long {
		const unsigned long long f = v & ~63ull;
		return f > k_first ? f : k_first;
	};

	// resampler table access and multiply-add shared by P6 and the flush-overrun epilogue
	// all-float model: the converter's products are rounded one by one as SampleRateConverter<float> does, which
	// makes the output samples bit-identical to the float reference; in fp64 / mixed they may fuse
	auto src_tap = [&](unsigned idx) -> SrcTap<ST> {
		if constexpr (kSrcHOnly<CT, ST, U>) {
			const ST* hh = reinterpret_cast<const ST*>(sm.src) + idx;
			SrcTap<ST> t;
			t.h = hh[0];
			t.dh = hh[1] - hh[0];
			return t;
		} else {
			return sm.src[idx];
		}
	};
	// c + a * b.  All-float model: the product rounded on its own, as SampleRateConverter<float> does.  fp64 / mixed:
	// ONE fused operation, spelled out so that every row of a workgroup is computed the same way (left to the
	// compiler, the unrolled rows came out fused or not by position: identical utterances differed in the last bit
	// depending on their row).
	auto mad = [](ST a, ST b, ST c) -> ST {
		if constexpr (sizeof(CT) == 4) return c + rmul(a, b);
		else if constexpr (sizeof(ST) == 4) return __builtin_fmaf(a, b, c);
		else return __builtin_fma(a, b, c);
	};

	// P6: SampleRateConverter::dataEmpty (SampleRateConverter.h:295-416) evaluated per output sample
	// A pass covers 64 output samples of UG = U / kP6Groups utterances.  In float all four rows of a workgroup go in one
	// pass (the coefficient of a tap is formed once for them); in double such a pass is longer than a whole tick of the
	// tube (one wavefront was still busy with it when everybody else had finished: 375 / 511 cycles per step in mixed /
	// fp64 against 260 for the tube), so the rows are split over two passes that different wavefronts pick up, each
	// forming the coefficients again (four passes of one row in fp64 measured 14 % slower than two of two).
	constexpr int kP6Groups = (sizeof(CT) == 8 && U == 4) ? 2 : 1;
	constexpr int UG = U / kP6Groups;
	auto stage_p6 = [&](int c, int pass_and_group) {
		const int pass = pass_and_group / kP6Groups;
		const int u0 = (pass_and_group % kP6Groups) * UG; // first utterance of this pass
		// Output sample ko of EVERY utterance has the same time register (t = ko * inc), hence the same
		// filter phase: the polyphase coefficient of a tap is formed once and applied to the pass's rows.
		// output index range of the chunk.  With several rows stage_bounds has it ready, one tick earlier (by
		// running remainder or, shape by shape, by division); with one row the (emulated 64-bit) divisions done
		// here measured faster than a stage of their own, with either form of it.
		uint64_t k_lo;
		uint64_t k_hi[UG];
		uint64_t k_hi_max = 0;
		if constexpr (U > 1) {
			const unsigned long long* kb = sm.kb + (c & 1) * (U + 1);
			k_lo = kb[0];
#pragma unroll
			for (int u = 0; u < UG; ++u) {
				k_hi[u] = kb[1 + u0 + u];
				k_hi_max = k_hi[u] > k_hi_max ? k_hi[u] : k_hi_max;
			}
		} else {
			const Extent e = sm.ext[0];
			const uint64_t n0 = e.step_base + static_cast<uint64_t>(c) * C;
			k_lo = grid_floor(((n0 << 16) + k.time_inc - 1) / k.time_inc, e.k_first);
			k_hi[0] = 0;
			if (valid_in(0, c) >= 0) {
				const bool last = c == e.nchunks - 1;
				const uint64_t filled = last ? e.step_base + e.steps + (kFinal ? 2ull * k.pad : 0ull) : n0 + C;
				const uint64_t avail = ((filled << 16) + k.time_inc - 1) / k.time_inc;
				k_hi[0] = last ? avail : grid_floor(avail, e.k_first);
			}
			k_hi_max = k_hi[0];
		}
		const uint64_t ko = k_lo + static_cast<uint64_t>(pass) * 64 + hl;
		if (ko >= k_hi_max) return;
		const uint64_t t = ko * k.time_inc;
		const int base = static_cast<int>(t >> 16) - k.pad; // ring index p holds internal sample p - pad
		const unsigned frac = static_cast<unsigned>(t & 0xFFFFu);
		ST acc[UG];
#pragma unroll
		for (int u = 0; u < UG; ++u) acc[u] = ST(0);
		const ST* xg = sm.x + u0 * XRS; // the pass's rows
		// one tap for all rows, the rows' samples given; the float resampler of the mixed path takes the rows in pairs (v_pk_fma_f32)
		auto tapv = [&](const ST (&xs)[UG], ST coef) {
			if constexpr (sizeof(CT) == 8 && sizeof(ST) == 4 && U >= 2) {
				using F2 = float __attribute__((ext_vector_type(2)));
#pragma unroll
				for (int u = 0; u < UG; u += 2) {
					const F2 xv = {xs[u], xs[u + 1]};
					F2 av = {acc[u], acc[u + 1]};
					av = __builtin_elementwise_fma(xv, F2{coef, coef}, av);
					acc[u] = av.x;
					acc[u + 1] = av.y;
				}
			} else {
#pragma unroll
				for (int u = 0; u < UG; ++u) acc[u] = mad(xs[u], coef, acc[u]);
			}
		};
		auto tap = [&](int ri, ST coef) {
			ST xs[UG];
#pragma unroll
			for (int u = 0; u < UG; ++u) xs[u] = xg[u * XRS + ri];
			tapv(xs, coef);
		};
		if (k.upsampling) {
			const unsigned l = frac >> 8, m = frac & 0xFFu;
			const ST interp = static_cast<ST>(m) / ST(256);
			const int lo = (base - (kSrcZeroCrossings - 1)) & (XR - 1); // the run base - 12 .. base + 13 starts here (mirror behind the end)
			const unsigned nfrac = (~frac) & 0xFFFFu;
			const unsigned l2 = nfrac >> 8, m2 = nfrac & 0xFFu;
			const ST interp2 = static_cast<ST>(m2) / ST(256);
			if constexpr (sizeof(CT) == 4) {
			// A wing's reads all go out before its arithmetic starts (13 table entries, 13 samples of every row): taken
			// tap by tap, every tap waited for its own LDS round trip -- 26 of them in a row made this pass ~9000 cycles
			// long, three quarters of a tick, and the tick could not end before it (profiles/r02_tick_trace_*.txt).
			auto wing = [&](unsigned lbase, ST ip, int x0, int xstep) {
				constexpr int kZ = kSrcZeroCrossings;
				SrcTap<ST> cf[kZ];
				ST xv[kZ][UG];
#pragma unroll
				for (int j = 0; j < kZ; ++j) cf[j] = src_tap(lbase + 256 * j);
#pragma unroll
				for (int j = 0; j < kZ; ++j) {
#pragma unroll
					for (int u = 0; u < UG; ++u) xv[j][u] = xg[u * XRS + x0 + xstep * j];
				}
				// (a compiler barrier for memory operations: without it the reads are sunk back to their uses)
				asm volatile("" ::: "memory");
#pragma unroll
				for (int j = 0; j < kZ; ++j) tapv(xv[j], mad(cf[j].dh, ip, cf[j].h));
			};
			// The 26 coefficients depend on frac alone, frac on ko mod (a.src_phase_mask + 1): a plan that has tabulated them by
			// output phase (a.src_phase, device memory) hands a lane its record -- seven 16-byte loads at immediate offsets from
			// one address, on the vector-memory path, which a tick leaves idle -- and the wings read samples only: no table
			// entry from LDS, no address arithmetic for 26 of them, no coefficient formed.  The host made each entry with the
			// operations of mad(cf.dh, ip, cf.h) on the plan's own float tables (design_src_phase_table), so the bits are these.
			// The wing's rule holds: every read is out before the arithmetic starts, the record's with the first wing's samples.
			if constexpr (kSrcPhaseTable) {
				if (a.src_phase != nullptr) {
					using F4 = float __attribute__((ext_vector_type(4)));
					constexpr int kZ = kSrcZeroCrossings;
					static_assert(kSrcPhaseRecord % 4 == 0 && 2 * kZ <= kSrcPhaseRecord, "a record: both wings in whole 16-byte loads");
					const F4* rec = reinterpret_cast<const F4*>(a.src_phase + static_cast<size_t>(static_cast<unsigned>(ko) & a.src_phase_mask) * kSrcPhaseRecord);
					F4 cq[kSrcPhaseRecord / 4];
#pragma unroll
					for (int q = 0; q < kSrcPhaseRecord / 4; ++q) cq[q] = rec[q];
					auto wing_samples = [&](int c0, int x0, int xstep) {
						ST xv[kZ][UG];
#pragma unroll
						for (int j = 0; j < kZ; ++j) {
#pragma unroll
							for (int u = 0; u < UG; ++u) xv[j][u] = xg[u * XRS + x0 + xstep * j];
						}
						asm volatile("" ::: "memory");
#pragma unroll
						for (int j = 0; j < kZ; ++j) tapv(xv[j], static_cast<ST>(cq[(c0 + j) >> 2][(c0 + j) & 3]));
					};
					wing_samples(0, lo + (kZ - 1), -1);
					wing_samples(kZ, lo + kZ, 1);
				} else {
					wing(l, interp, lo + (kSrcZeroCrossings - 1), -1);
					wing(l2, interp2, lo + kSrcZeroCrossings, 1);
				}
			} else {
			wing(l, interp, lo + (kSrcZeroCrossings - 1), -1);
			wing(l2, interp2, lo + kSrcZeroCrossings, 1);
			}
			} else if constexpr (U >= 4) {
				// the double paths: a wing in groups of a few taps, a group's reads before its arithmetic (whole wings
				// spill there; tap by tap every tap waits for its own LDS round trip)
				constexpr int kG = 4; // (groups of 2 / 7: within 1 % of 4)
				auto wing_groups = [&](unsigned lbase, ST ip, int x0, int xstep) {
#pragma unroll
					for (int j0 = 0; j0 < kSrcZeroCrossings; j0 += kG) {
						SrcTap<ST> cf[kG];
						ST xv[kG][UG];
#pragma unroll
						for (int g = 0; g < kG; ++g) {
							if (j0 + g < kSrcZeroCrossings) {
								cf[g] = src_tap(lbase + 256 * (j0 + g));
#pragma unroll
								for (int u = 0; u < UG; ++u) xv[g][u] = xg[u * XRS + x0 + xstep * (j0 + g)];
							}
						}
						asm volatile("" ::: "memory");
#pragma unroll
						for (int g = 0; g < kG; ++g) {
							if (j0 + g < kSrcZeroCrossings) tapv(xv[g], mad(cf[g].dh, ip, cf[g].h));
						}
					}
				};
				wing_groups(l, interp, lo + (kSrcZeroCrossings - 1), -1);
				wing_groups(l2, interp2, lo + kSrcZeroCrossings, 1);
			} else {
#pragma unroll
			for (int j = 0; j < kSrcZeroCrossings; ++j) {
				const SrcTap<ST> cf = src_tap(l + 256 * j);
				const ST coef = mad(cf.dh, interp, cf.h);
				tap(lo + (kSrcZeroCrossings - 1 - j), coef);
			}
#pragma unroll
			for (int j = 0; j < kSrcZeroCrossings; ++j) {
				const SrcTap<ST> cf = src_tap(l2 + 256 * j);
				const ST coef = mad(cf.dh, interp2, cf.h);
				tap(lo + kSrcZeroCrossings + j, coef);
			}
			}
		} else {
			unsigned ph = static_cast<unsigned>(rint(static_cast<CT>(frac) * CT(k.src_ratio)));
			unsigned ii;
			int j = 0;
			while ((ii = (ph >> 8)) < static_cast<unsigned>(kSrcFilterLength)) {
				const SrcTap<ST> cf = src_tap(ii);
				const ST coef = mad(cf.dh, static_cast<ST>(ph & 0xFFu) / ST(256), cf.h);
				tap((base - j) & (XR - 1), coef);
				++j;
				ph += k.phase_inc;
			}
			ph = static_cast<unsigned>(rint(static_cast<CT>((~frac) & 0xFFFFu) * CT(k.src_ratio)));
			j = 0;
			while ((ii = (ph >> 8)) < static_cast<unsigned>(kSrcFilterLength)) {
				const SrcTap<ST> cf = src_tap(ii);
				const ST coef = mad(cf.dh, static_cast<ST>(ph & 0xFFu) / ST(256), cf.h);
				tap((base + 1 + j) & (XR - 1), coef);
				++j;
				ph += k.phase_inc;
			}
		}
#pragma unroll
		for (int u = 0; u < UG; ++u) {
			const float y = (ko < k_hi[u]) ? static_cast<float>(acc[u]) : 0.0f;
			// (a stream's launch numbers its samples from its own first one)
			const uint64_t kout = ko - sm.ext[u0 + u].k_first;
			if (ko < k_hi[u] && kout < a.audio_stride) a.audio[GVTM_ROW_UTT(u0 + u, (group * U + u0 + u)) * a.audio_stride + kout] = y;
			// maximum of every 16-lane row by DPP rotations (lanes that have left the pass supply 0), one LDS atomic per row
			// and utterance.  (The butterfly over the whole wavefront with __shfl_xor was six ds_bpermute round trips in a
			// row per utterance -- 24 dependent LDS round trips at the end of a pass, most of its ~7800 cycles.)
			// row_rotate<N> hands lane i the value of lane i - N (mod 16): by 15, 14, 12 and 8 a lane takes in lanes i + 1,
			// i + 2, i + 4 and i + 8, the following lanes, so the row's first lane ends up with the maximum of the whole
			// row -- also of a row that is cut short, whose lanes that left are its last ones (the end of every launch of
			// a stream, and of its first emission up to the aligned grid).  (By 1, 2, 4 and 8 the first lane of a cut row
			// took in the lanes that had left and published its own sample alone.)
			float mx = fabsf(y);
			mx = fmaxf(mx, row_rotate<15>(mx));
			mx = fmaxf(mx, row_rotate<14>(mx));
			mx = fmaxf(mx, row_rotate<12>(mx));
			mx = fmaxf(mx, row_rotate<8>(mx));
			if ((hl & 15) == 0) atomicMax(&sm.peak[u0 + u], __float_as_uint(mx));
		}
	};

	// -------------------------------------------------------------------------------------
	// serial stages (a 16-lane row per utterance)

	// I: Controller::synthesize's interpolation (Controller.cpp:294-311).  Lane L owns parameter L and
	// runs `ahead` chunks in front of the tick so that its consumer stage finds it one tick later:
	// pitch/glotVol/aspVol feed P2a (2 ahead), the frication parameters P2c (1 behind), radii and
	// velum P2b (2 behind).
	auto stage_bounds = [&](int t) {
		// output sample ranges of the chunk the resampler handles NEXT tick (chunk t - 5): sample ko is
		// produced once its read position P = floor(ko * inc / 2^16) lies before the filled length
		if (lane <= U) {
			const int cc = t - 5;
			if (cc >= 0) {
				// (the rows of a workgroup share one output index range start: utterances of a stream that share a
				// workgroup have been pushed in lockstep, the host launches one row per workgroup otherwise)
				const Extent e = sm.ext[lane == 0 ? 0 : lane - 1];
				unsigned long long v = 0;
				if constexpr (kBoundsRecurrence) {
					// Lane 0 reports ceil((step_base + cc * C) * 2^16 / time_inc) of utterance 0 and lane 1 + u the same at
					// (cc + 1) * C of utterance u: bnd, which moves on by one chunk per tick (the other branch's two emulated 64-bit
					// divisions).  Only the end of an utterance's last chunk, no whole chunk away, is divided out: once per launch.
					if (lane == 0 || cc < e.nchunks - 1) {
						v = grid_floor(bnd.q, e.k_first);
					} else if (cc == e.nchunks - 1) {
						v = src_bounds_at(k.time_inc, e.step_base + e.steps + (kFinal ? 2ull * k.pad : 0ull)).q;
					}
					src_bounds_advance(bnd, SrcBoundsStep{sm.ticket[2], sm.ticket[3]}, k.time_inc);
				} else {
					const uint64_t n0 = e.step_base + static_cast<uint64_t>(cc) * C;
					if (lane == 0) {
						v = grid_floor(((n0 << 16) + k.time_inc - 1) / k.time_inc, e.k_first);
					} else if (valid_in(lane - 1, cc) >= 0) {
						const bool last = cc == e.nchunks - 1;
						const uint64_t filled = last ? e.step_base + e.steps + (kFinal ? 2ull * k.pad : 0ull) : n0 + C;
						const uint64_t avail = ((filled << 16) + k.time_inc - 1) / k.time_inc;
						v = last ? avail : grid_floor(avail, e.k_first);
					}
				}
				sm.kb[(cc & 1) * (U + 1) + lane] = v;
			}
		}
	};

	auto stage_interp = [&](int t) {
		if (rowp >= U) return;
		const int u = rowp;
		const int c = t + (Lp < 3 ? 2 : (Lp < 7 ? -1 : -2));
		const int valid = valid_in(u, c);
		if (valid <= 0) return;
		if constexpr (TARGETS) {
			// The second driver: the moving average of the lane's target list, step by step.  Blocks of four steps as below:
			// the cursors' bookkeeping only runs for a block in which some lane's cursor moves (a point enters, or leaves N
			// steps later); every other block is four times {two double additions, a multiplication, a conversion, a store}.
			// A partial last block runs on: no cursor passes the end of its list, and the extra rows are never read.
			// (the filter's length and reciprocal through closures whose other arm is never instantiated: this stage's own closure
			// carries the voice's two in the kernels of several voices only, and is what it was in the others)
			[[maybe_unused]] const auto tg_length = [&]() -> int64_t { if constexpr (VOICES) return tgv_N; else return a.tg_N; };
			[[maybe_unused]] const auto tg_inverse = [&]() -> double { if constexpr (VOICES) return tgv_invN; else return a.tg_invN; };
			float* out = sm.prm + at_prm(c & 1, u) + Lp;
			const int64_t first = tg_base + static_cast<int64_t>(c) * C;
			for (int s0 = 0; s0 < valid; s0 += 4) {
				if (__builtin_expect(__any(targets_moves(tg, first + s0, 4)), 0)) {
#pragma unroll
					for (int q = 0; q < 4; ++q) {
						targets_move(tg, first + s0 + q, a.tg_steps, a.tg_values, tg_length());
						out[(s0 + q) * kPrm] = targets_step(tg, tg_inverse());
					}
				} else {
#pragma unroll
					for (int q = 0; q < 4; ++q) out[(s0 + q) * kPrm] = targets_step(tg, tg_inverse());
				}
			}
			return;
		}
		const int last = sm.ext[u].last_frame;
		const float* __restrict__ P = a.params + GVTM_ROW_UTT(u, (group * U + u)) * a.max_frames * 16;
		float* out = sm.prm + at_prm(c & 1, u) + Lp;
		const uint32_t cs = k.control_steps;
		const float coef = k.interp_coef;
		auto one = [&](int s) {
			if (ip_j == 0) {
				// restart from the frame value, delta towards the next frame (Controller.cpp:297-300)
				ip_cur = ip_this;
				ip_delta = interp_delta(ip_next, ip_cur, coef);
			}
			out[s * kPrm] = ip_cur;
			ip_cur = interp_advance(ip_cur, ip_delta); // Controller.cpp:308-310
			if (++ip_j == cs) {
				ip_j = 0;
				++ip_frame;
				ip_this = ip_next;
				ip_next = ip_next2;
				const int f = ip_frame + 2;
				ip_next2 = P[static_cast<size_t>(f < last ? f : last) * 16 + Lp];
			}
		};
		// Blocks of four steps: inside a frame a step is a store and an addition; the frame-boundary bookkeeping only runs
		// for a block in which some lane of the wavefront starts or ends a frame (one block in 20 to 40).  A partial last
		// block runs on (the state is not used after an utterance's last chunk; the extra rows are never read).
		static_assert(C % 4 == 0, "interpolation works in blocks of four steps");
		for (int s0 = 0; s0 < valid; s0 += 4) {
			if (__builtin_expect(__any(ip_j == 0 || ip_j + 4 >= cs), 0)) {
#pragma unroll
				for (int q = 0; q < 4; ++q) one(s0 + q);
			} else {
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					out[(s0 + q) * kPrm] = ip_cur;
					ip_cur = interp_advance(ip_cur, ip_delta);
				}
				ip_j += 4;
			}
		}
	};

	// S1: oscillator phase (mod0 recurrence, WavetableGlottalSource.h:196-199, :265-272) and the
	// noise generator + one-zero low-pass (NoiseSource.h:40-44, NoiseFilter.h:63-68)
	auto stage_s1 = [&](int c) {
		const int u = urow;
		const int valid = valid_in(u, c);
		const bool writer = (L == 0) && (urow < U) && (U >= 4 || row < U);
		const CT* inc = sm.inc + ((c & 1) * U + u) * C;
		CT* pos = sm.pos + ((c & 1) * U + u) * 2 * C;
		CT* noise = sm.noise + ((c % 3) * U + u) * C;
		// Blocks of four steps: the increments of the next block are fetched while this one is
		// computed and results leave in wide stores.  No per-step bounds checks: a partial last block
		// just runs on (the state is never used after the utterance's last chunk).
		// Only the lane that owns an utterance's scan runs it: with every lane reading the increments and storing its
		// (unused) results into a dump area, this four-lane stage kept the LDS busy 16 cycles per step, 9 of them bank
		// conflicts (profiles/r02_stage_lds_cycles.md).
		static_assert(C % 4 == 0, "scan works in blocks of four steps");
		if (kMaskedSerial && !writer) return;
		CT* pos_w = writer ? pos : sm.dump + lane;
		CT* noise_w = writer ? noise : sm.dump + 64 + lane;
		const int pos_stride = writer ? 2 : 0, noise_stride = writer ? 1 : 0;
		// one-shot launches: the noise samples come from the plan's table (the decimator pass reads them), every utterance
		// drawing the same sequence; a stream generates them here
		// (float model only: with the table the double paths measured 7-10 % SLOWER at four utterances per workgroup --
		// their fp64 conversion passes P2a / P2c take 60 % longer when the scan wavefront joins the helpers that early)
		const bool gen_noise = !kNoiseTable || a.noise_lp == nullptr;
		// (two copies of the loop: the choice between generating the noise samples and leaving them to the table is made
		// once, not per step)
		auto scan = [&](auto with_noise) {
		CT dn[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) dn[q] = inc[q];
		for (int s0 = 0; s0 < valid; s0 += 4) {
			CT d[4];
#pragma unroll
			for (int q = 0; q < 4; ++q) d[q] = dn[q];
			{
				const int sn = (s0 + 4 < C) ? s0 + 4 : s0;
#pragma unroll
				for (int q = 0; q < 4; ++q) dn[q] = inc[sn + q];
			}
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				CT p0 = sc_pos + d[q];
				CT p1 = p0 + d[q];
				// mod0 (WavetableGlottalSource.h:265-272).  The increment is positive, so p1 <= 511 means
				// neither half step wrapped; the wrap path runs only when some lane of the wavefront needs it.
				if (__builtin_expect(__any(p1 > CT(511.0)), 0)) {
					if (p0 > CT(511.0)) p0 -= CT(512.0);
					p1 = p0 + d[q];
					if (p1 > CT(511.0)) p1 -= CT(512.0);
				}
				sc_pos = p1;
				pos_w[pos_stride * (s0 + q)] = p0;
				pos_w[pos_stride * (s0 + q) + 1] = p1;
				if constexpr (decltype(with_noise)::value) {
					sc_seed = noise_advance(sc_seed);
					const CT white = static_cast<CT>(sc_seed - 0.5); // getSample() returns double; NoiseFilter<TFloat> adds in TFloat
					const CT lp = white + sc_prev;
					sc_prev = white;
					noise_w[noise_stride * (s0 + q)] = lp;
				}
			}
		}
			};
		if constexpr (!kNoiseTable) scan(std::true_type{});
		else if (gen_noise) scan(std::true_type{});
		else scan(std::false_type{});
	};

	// F1: band-pass (BandpassFilter.h:114-122) -> injection of every section for the tube lanes,
	// and the throat low-pass (Throat.h:76-85)
	auto stage_f1 = [&](int c) {
		const int u = urow;
		const int valid = valid_in(u, c);
		const bool active = U >= 4 || row < U;
		// (read cursors as opaque element indices into the LDS block, see the tube stage: otherwise every read of a block
		// of steps gets its own address addition, the region offsets not fitting an immediate)
		const CT* const lds0 = reinterpret_cast<const CT*>(smem_raw);
		unsigned iu = static_cast<unsigned>(sm.usg + at_usg(c & 1, u) - lds0), ifr = static_cast<unsigned>(sm.fr + at_fr(c & 1, u) - lds0);
		asm volatile("" : "+v"(iu), "+v"(ifr));
		const CT* usg = lds0 + iu;
		const CT* fr = lds0 + ifr;
		CT* inj = (kLaneRec ? sm.kl : sm.inj) + at_inj(c & 1, u);
		CT* thy = sm.thy + (static_cast<size_t>(c % 3) * U + u) * C;
		// lane 0 forwards the tube input, lanes 1..8 scale the band-passed noise by FC1..FC8
		const int Lf = lane & 15;
		const bool inj_lane = active && Lf < 9 && (kRowView || lane < 16);
		const int my_section = Lf - 1; // compact record: the frication tap this lane scales (FC1..FC8 = taps 0..7 on lanes 1..8)
		const int tap_idx = (Lf >= 1 && Lf <= 8) ? Lf - 1 : kFr - 1; // dense record: my tap, or the padding slot (always 0)
		const CT tb0 = GVTM_KF(kKfThroatB0, throat_b0), ta1 = GVTM_KF(kKfThroatA1, throat_a1), tgain = GVTM_KF(kKfThroatGain, throat_gain);
		// lanes that own no result store into the dump area (no exec-mask juggling in the loop)
		if (kMaskedSerial && !inj_lane) return; // (the other lanes used to read every input and store into a dump area: LDS time)
		CT* inj_w = inj_lane ? inj + Lf : sm.dump + lane;
		CT* thy_w = (inj_lane && Lf == 0) ? thy : sm.dump + 64 + lane;
		const int inj_stride = inj_lane ? kInjLen : 0, thy_stride = (inj_lane && Lf == 0) ? 1 : 0;
		// Blocks of four steps (float): the planes are read four values at a time (wide LDS reads, all of a block's reads in
		// flight together) one block ahead of their use, the filter memories rotate through registers instead of being
		// copied (an even number of steps per block brings them back), and the four throat samples leave in one store.
		// A partial last block runs on over stale inputs (the states are never used after the utterance's last chunk,
		// only its last chunk can be partial, and what is written beyond its end is never read).
		// (blocks of two in double: two blocks of seven planes are 56 registers there already)
		constexpr int kB = sizeof(CT) == 8 ? 2 : 4;
		static_assert(C % kB == 0, "pre-tube filters work in blocks of steps");
		struct Blk { CT u[kB], sig[kB], thr[kB], b0[kB], a1[kB], a2[kB], tap[kB]; };
		auto fetch = [&](int s0) {
			Blk r;
			const CT* up = usg + s0;
#pragma unroll
			for (int q = 0; q < kB; ++q) {
				r.u[q] = up[kF1U * C + q]; r.sig[q] = up[kF1Sig * C + q]; r.thr[q] = up[kF1Thr * C + q];
				r.b0[q] = up[kF1B0 * C + q]; r.a1[q] = up[kF1A1 * C + q]; r.a2[q] = up[kF1A2 * C + q];
				const CT* f = fr + (s0 + q) * kFr;
				if constexpr (kFrCompact) {
					const unsigned d = static_cast<unsigned>(my_section - *reinterpret_cast<const int*>(f + kFrFirst));
					r.tap[q] = f[d < 2u ? d : 2u]; // my share, or the zero
				} else {
					r.tap[q] = f[tap_idx];
				}
			}
			return r;
		};
		CT injv[kB]; // (block layout: a block's injection values leave in one store)
		auto step = [&](const Blk& r, int q, CT& x1, CT& x2, CT& y1, CT& y2, int s, CT& thy_out) {
			// y = b0 (x - x2) - a1 y1 - a2 y2 (BandpassFilter.h:114-122); x2 / y2 are overwritten by the new x / y
			const CT fric = rmul(r.b0[q], r.sig[q] - x2) - rmul(r.a1[q], y1) - rmul(r.a2[q], y2);
			x2 = r.sig[q]; y2 = fric;
			const CT ty = rmul(tb0, r.thr[q]) - rmul(ta1, thr_y1);
			thr_y1 = ty;
			// setFricationTaps' eight taps; a lane whose section gets no share still forms 0 * fric, a signed zero
			if constexpr (kBlockRec) injv[q] = (Lf == 0) ? r.u[q] : r.tap[q] * fric;
			else inj_w[inj_stride * s] = (Lf == 0) ? r.u[q] : r.tap[q] * fric;
			thy_out = ty * tgain;
		};
		if (valid > 0) {
			auto process = [&](const Blk& cb, int s0) {
				CT ty[kB];
#pragma unroll
				for (int q = 0; q < kB; q += 2) {
					step(cb, q, bp_x1, bp_x2, bp_y1, bp_y2, s0 + q, ty[q]);              // afterwards x2 / y2 hold the newest values ...
					step(cb, q + 1, bp_x2, bp_x1, bp_y2, bp_y1, s0 + q + 1, ty[q + 1]);  // ... so the roles swap, and swap back
				}
				if constexpr (kBlockRec) {
					using F4 = float __attribute__((ext_vector_type(4)));
					static_assert(!kBlockRec || (kB == 4 && kMaskedSerial), "block layout: float, blocks of four steps, owning lanes only");
					*reinterpret_cast<F4*>(sm.kl + at_kl(c & 1, u) + kl_index(s0, kLrInj + Lf)) = F4{injv[0], injv[1], injv[2], injv[3]};
				}
				CT* tw = thy_w + thy_stride * s0;
				if (!kMaskedSerial || Lf == 0) {
#pragma unroll
					for (int q = 0; q < kB; ++q) tw[thy_stride ? q : 0] = ty[q];
				}
			};
			if constexpr (kBlockRec) {
				// two blocks per iteration, a register set each (no copies of the prefetched planes: eight 64-bit moves per
				// block): 4096 x 500 x SectionDelay 1 13.13 -> 12.63 ms, SectionDelay 2 x 2000 94.7 -> 94.0
				Blk ba = fetch(0);
				int s0 = 0;
				for (; s0 + kB < valid; s0 += 2 * kB) {
					const Blk bb = fetch(s0 + kB);
					process(ba, s0);
					ba = fetch(s0 + 2 * kB); // past the chunk: the next LDS rows, never used
					process(bb, s0 + kB);
				}
				if (s0 < valid) process(ba, s0);
			} else {
				Blk nb = fetch(0);
				for (int s0 = 0; s0 < valid; s0 += kB) {
					const Blk cb = nb;
					nb = fetch(s0 + kB); // past the chunk: the next LDS rows, never used
					process(cb, s0);
				}
			}
		}
	};

	// F2 where filter_split_f2() says so: the same operations as stage_f2's serial loop below, but only the recurrence runs
	// on the two lanes of a row.  The radiation filter is oy = (a x - a x1) + a y1 with every product rounded, x being
	// (1 + k) * top: the difference d = a x[n] - a x[n-1] needs steps n and n - 1 of the tube's output alone, and the
	// previous step's product has the same operands, hence the same bits, as when that step formed it.  Three passes of
	// the one wavefront over the chunk, separated by program order alone (a wavefront's LDS operations complete in order):
	//   1  all 64 lanes, one item per (row, mouth | nose, step): d, IN PLACE over the tube's output in sm.ox (this slot has
	//      no other reader, and the tube writes the other slot this tick).  An item reads its left neighbour's input, so
	//      the blocks of 64 items go from the highest down.  Step 0 stores a x[0] alone;
	//   2  lanes 0 and 1 of a row: y[n] = d[n] + a y[n-1], four steps per 16-byte read and write, in place again.  The lane
	//      subtracts a * (the x its state carries) from d[0] first, and ends with the state the serial form leaves: the
	//      last valid step's x (read before pass 1 overwrites it) and y.  A partial last block runs on, as below;
	//   3  all 64 lanes, one item per (row, step): (mouth + nose) + throat into the ring and its mirror, the steps below the
	//      row's count only.
	auto stage_f2_split = [&]([[maybe_unused]] int c, [[maybe_unused]] int valid) {
		if constexpr (kSplitF2) {
#pragma clang fp contract(off)
		using F4 = float __attribute__((ext_vector_type(4)));
		static_assert(!kSplitF2 || (kBlockRec && kMaskedSerial && kRowView && C % 4 == 0), "split post-tube filters: float, block record, row view");
		constexpr int kRows = U < 4 ? U : 4;  // utterances of this wavefront
		const int ub = U >= 4 ? sub * 4 : 0;  // the first of them
		CT* const oxs = sm.ox + (static_cast<size_t>(c & 1) * U + ub) * C * 2; // [row][mouth | nose][C]
		const CT* const opks = sm.opk + (static_cast<size_t>(c % 3) * U + ub) * C;
		const CT* const thys = sm.thy + (static_cast<size_t>(c % 3) * U + ub) * C;
		// (the lane as an opaque value: the masks and cursors this stage derives from it are formed again every tick.  Left to
		// the compiler they were kept in scalar registers from tick to tick, across the helper passes' loop, which spills
		// them: 119 against 108 spilled SGPRs and 35 more v_readlane / v_writelane in that loop's own code, and the flagship
		// was 0.5 % SLOWER than without the split.  The constants stay kernel arguments: from their LDS copy, which no tick
		// could keep either, the tube loop ran 141 instead of 136 cycles per step and the flagship +2.9 %;
		// profiles/filter_split_ab.md)
		const CT ra_m = GVTM_KF(kKfMouthARad, mouth_a_rad), ra_n = GVTM_KF(kKfNoseARad, nose_a_rad);
		const CT opk_nose = CT(1.0) + GVTM_KF(kKfNasalK5, nasal_k[5]);
		int ln = lane;
		asm volatile("" : "+v"(ln));
		const int L = ln & 15, row = ln >> 4;
		const bool owner = (U >= 4 || row < U) && L < 2 && valid > 0; // the lanes of pass 2
		CT x_last = CT(0.0);
		if (owner) x_last = rmul(L == 0 ? opks[row * C + valid - 1] : opk_nose, oxs[(row * 2 + L) * C + valid - 1]);
		// pass 1 (lane = step, row after row: which filter an item belongs to is uniform, and its addresses are the lane's
		// cursor plus immediates)
		CT* const lds0 = reinterpret_cast<CT*>(smem_raw);
		unsigned ix = static_cast<unsigned>(oxs - lds0) + ln, iq = static_cast<unsigned>(opks - lds0) + ln, it = static_cast<unsigned>(thys - lds0) + ln;
		const int back = ln > 0 ? 1 : 0; // (step 0 of a chunk has no left neighbour: it reads itself, and stores a x[0])
		unsigned ixb = ix - back, iqb = iq - back;
		asm volatile("" : "+v"(ix), "+v"(iq), "+v"(it), "+v"(ixb), "+v"(iqb));
		CT* const px = lds0 + ix;
		const CT* const pq = lds0 + iq;
		const CT* const pt = lds0 + it;
		const CT* const pxb = lds0 + ixb; // the cursors one step back
		const CT* const pqb = lds0 + iqb;
#pragma unroll
		for (int sb = ((C - 1) / 64) * 64; sb >= 0; sb -= 64) { // (from the highest 64 steps down: step sb reads step sb - 1)
			if (C - sb < 64 && ln >= C - sb) continue;
			const CT* const pxl = sb > 0 ? px - 1 : pxb;
			const CT* const pql = sb > 0 ? pq - 1 : pqb;
			const bool left = sb > 0 || ln > 0;
#pragma unroll
			for (int r = 0; r < 2 * kRows; ++r) { // r = 2 * row + (0 mouth | 1 nose)
				const int o = r * C + sb;
				const CT x = px[o], xp = pxl[o];
				CT p, pp;
				if (r & 1) {
					p = rmul(ra_n, rmul(opk_nose, x)); pp = rmul(ra_n, rmul(opk_nose, xp));
				} else {
					const int oq = (r >> 1) * C + sb;
					p = rmul(ra_m, rmul(pq[oq], x)); pp = rmul(ra_m, rmul(pql[oq], xp));
				}
				px[o] = left ? p - pp : p;
			}
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		// pass 2
		if (owner) {
			const CT ra = L == 0 ? ra_m : ra_n;
			// (the cursor as an opaque element index, see the tube stage: the block offsets become immediates)
			unsigned id = static_cast<unsigned>(oxs + (row * 2 + L) * C - lds0);
			asm volatile("" : "+v"(id));
			F4* pd = reinterpret_cast<F4*>(lds0 + id);
			CT y1 = rad_y1;
			auto run = [&](const F4& d) {
				F4 y;
				y.x = d.x + rmul(ra, y1);
				y.y = d.y + rmul(ra, y.x);
				y.z = d.z + rmul(ra, y.y);
				y.w = d.w + rmul(ra, y.z);
				y1 = y.w;
				return y;
			};
			F4 da = pd[0];
			da.x = da.x - rmul(ra, rad_x1);
			int s0 = 0;
			for (; s0 + 4 < valid; s0 += 8) {
				const F4 db = pd[1];
				pd[0] = run(da);
				da = pd[2]; // past the chunk: the next LDS rows, never used
				pd[1] = run(db);
				pd += 2;
			}
			if (s0 < valid) pd[0] = run(da);
			rad_x1 = x_last;
			rad_y1 = y1;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		// pass 3 (lane = step, row after row)
		const bool dbg = GVTM_KERNEL_TAPS && a.debug_taps != nullptr;
#pragma unroll
		for (int sb = 0; sb < C; sb += 64) {
			if (C - sb < 64 && ln >= C - sb) continue;
			const int s = sb + ln;
#pragma unroll
			for (int r = 0; r < kRows; ++r) {
				const int uu = ub + r;
				const CT sample = (px[2 * r * C + sb] + px[(2 * r + 1) * C + sb]) + pt[r * C + sb]; // (mouth + nose) + throat (VocalTractModel0.h:639-441)
				if (s < valid_in(uu, c)) {
					const unsigned slot = (static_cast<uint32_t>(sm.ext[uu].step_base) + static_cast<uint32_t>(c) * C + s) & (XR - 1); // ring slots go by the stream's sample number
					ST* xr = sm.x + uu * XRS;
					xr[slot] = static_cast<ST>(sample);
					if (slot < static_cast<unsigned>(kXMirror)) xr[XR + slot] = static_cast<ST>(sample); // the ring's first kXMirror samples a second time behind its end
					if (dbg) a.debug_taps[(GVTM_ROW_UTT(uu, (group * U + uu)) * a.max_frames * k.control_steps + static_cast<uint32_t>(c) * C + s) * 8 + 7] = sample;
				}
			}
		}
		}
	};

	// F2: radiation high-pass at mouth and nose (RadiationFilter.h:68-79), their sum and the throat
	// contribution (VocalTractModel0.h:639-441) -> internal-rate ring read by the resampler
	auto stage_f2 = [&](int c) {
		const int u = urow;
		const int valid = valid_in(u, c);
		if constexpr (kSplitF2) {
			if (c >= 0 && c < max_chunks) stage_f2_split(c, valid); // (all 64 lanes, whatever their own row's chunk count)
		}
		if (valid < 0) return;
		const Extent e = sm.ext[u];
		const bool active = U >= 4 || row < U;
		const uint32_t n0 = static_cast<uint32_t>(e.step_base) + static_cast<uint32_t>(c) * C; // ring slots go by the stream's sample number
		const CT* ox = sm.ox + (static_cast<size_t>(c & 1) * U + u) * C * 2; // [mouth | nose][C]
		const CT* thy = sm.thy + (static_cast<size_t>(c % 3) * U + u) * C;
		ST* xr = sm.x + u * XRS;
		// lane 0 of the row filters the mouth, lane 1 the nose (the others mirror lane 1)
		const int which = L == 0 ? 0 : 1;
		const CT ra = L == 0 ? GVTM_KF(kKfMouthARad, mouth_a_rad) : GVTM_KF(kKfNoseARad, nose_a_rad);
		const bool x_owner = active && L == 0; // the lane that writes the ring; the others store into the dump area
		ST* const x_dump = reinterpret_cast<ST*>(sm.dump + 128 + lane);
		const bool dbg = GVTM_KERNEL_TAPS && a.debug_taps != nullptr && active && L == 0;
		// Blocks of four steps: the next block's inputs (two wide LDS reads) are in flight while this one is computed, and
		// the four samples leave in one store.  (One step per iteration made every step wait for an LDS round trip: the
		// role took as long as the tube.)  A partial last block runs on over stale inputs: only an utterance's last chunk
		// can be partial, its filter state is not used again and the flush zeros below overwrite the extra ring slots.
		if (kSplitF2 || (kMaskedSerial && !(active && L < 2))) {
			// (only the mouth and nose lanes of a row run the filters; the flush zeros below take the whole row)
			// (kSplitF2: stage_f2_split has run them)
		} else {
		const CT* po = ox + which * C;
		const CT* pt = thy;
		// lane-indexed tube record: the tube wavefront hands over the bare top of the end sections and the radiated part
		// (1 + k) * top (VocalTractModel0.h:628, :655) is formed here, k being the mouth's coefficient of the step or the
		// nose's constant one (two instructions less per step in the tube wavefront, whose chain is the longest)
		const CT* pq = kLaneRec ? sm.opk + (static_cast<size_t>(c % 3) * U + u) * C : thy;
		const CT opk_nose = CT(1.0) + GVTM_KF(kKfNasalK5, nasal_k[5]);
		static_assert(C % 4 == 0, "post-tube filters work in blocks of four steps");
		struct Blk2 { CT x[4], t[4], q[4]; };
		auto fetch2 = [&]() {
			Blk2 r;
#pragma unroll
			for (int q = 0; q < 4; ++q) { r.x[q] = po[q]; r.t[q] = pt[q]; if constexpr (kLaneRec) r.q[q] = pq[q]; }
			po += 4; pt += 4; pq += 4;
			return r;
		};
		auto process2 = [&](const Blk2& cb, int s0) {
			ST out[4];
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				CT xin = cb.x[q];
				if constexpr (kLaneRec) xin = rmul(L == 0 ? cb.q[q] : opk_nose, xin);
				// y = b0 x + b1 x1 - a1 y1 with b1 = a1 = -b0: the two negations are exact, so the three rounded
				// products combine as (a x - a x1) + a y1.  (Written without fneg: a negated operand makes the
				// compiler rebuild the product with the caller's contraction flag and fuse it.)
				const CT oy = (rmul(ra, xin) - rmul(ra, rad_x1)) + rmul(ra, rad_y1);
				rad_x1 = xin; rad_y1 = oy;
				CT sample = oy + from_right(oy); // lane 0: mouth + nose
				sample += cb.t[q];
				out[q] = static_cast<ST>(sample);
				if (dbg) a.debug_taps[(GVTM_ROW_UTT(u, (group * U + u)) * a.max_frames * k.control_steps + static_cast<uint32_t>(c) * C + s0 + q) * 8 + 7] = sample;
			}
			const unsigned slot = (n0 + s0) & (XR - 1); // n0 + s0 is a multiple of four: the block does not wrap
			ST* xw = x_owner ? xr + slot : x_dump;
#pragma unroll
			for (int q = 0; q < 4; ++q) xw[q] = out[q];
			// the ring's first kXMirror samples a second time behind its end
			ST* xm = (x_owner && slot < static_cast<unsigned>(kXMirror)) ? xr + XR + slot : x_dump + 4;
#pragma unroll
			for (int q = 0; q < 4; ++q) xm[q] = out[q];
		};
		if constexpr (kBlockRec) {
			// two blocks per iteration, a register set each (as the tube and the pre-tube filters; 4096 x 2000 x SectionDelay 2
			// 93.4 -> 93.0 ms, 512 x 2 s 2.51 -> 2.47, neutral elsewhere)
			Blk2 ba = fetch2();
			int s0 = 0;
			for (; s0 + 4 < valid; s0 += 8) {
				const Blk2 bb = fetch2();
				process2(ba, s0);
				ba = fetch2(); // past the chunk: the next LDS rows, never used
				process2(bb, s0 + 4);
			}
			if (s0 < valid) process2(ba, s0);
		} else {
			Blk2 nb = fetch2();
			for (int s0 = 0; s0 < valid; s0 += 4) {
				const Blk2 cb = nb;
				nb = fetch2(); // past the chunk: the next LDS rows, never used
				process2(cb, s0);
			}
		}
		}
		if (c == e.nchunks - 1 && active && kFinal) {
			// flushBuffer (SampleRateConverter.h:462-471): 2*pad zero samples follow the utterance
			for (int i = L; i < 2 * k.pad; i += 16) {
				const unsigned slot = (static_cast<uint32_t>(e.step_base) + e.steps + i) & (XR - 1);
				xr[slot] = ST(0);
				if (slot < static_cast<unsigned>(kXMirror)) xr[XR + slot] = ST(0);
			}
		}
	};

	// T: the waveguide (VocalTractModel0.h:565-661 / VocalTractModel2.h:626-669 / VocalTractModel4.h:671-745),
	// one section per lane; what a lane's two sides are comes from the layout table
	// Float with the block record: the tube lane's layout entry and plan constants are read ONCE (five dependent LDS round
	// trips at the start of every tick otherwise: 16 of the tube wavefront's 182 cycles per step, and with sixteen
	// wavefronts per workgroup the tube is the tick).  The tube wavefront runs a tick loop of its own, so only its path
	// carries the registers.  (In the double models, whose every wavefront sits at the register limit, the same hoist
	// measured slower: mixed +5.5 %.)
	constexpr bool kTubeHoist = kBlockRec;
	int t_packed = 0;
	CT t_damping = CT(0.0), t_mb0 = CT(0.0), t_ma1 = CT(0.0), t_nb0 = CT(0.0), t_na1 = CT(0.0), t_nk = CT(0.0);
	if (kTubeHoist && role == 0) {
		const int Lt0 = kTubePerWave ? lane : L;
		t_packed = reinterpret_cast<const int*>(sm.lanec + 72)[TL::kWaveWide ? (Lt0 < 48 ? Lt0 : 47) : (Lt0 & 15)];
		t_damping = CT(k.damping);
		t_mb0 = CT(k.mouth_b0_refl); t_ma1 = CT(k.mouth_a1_refl);
		t_nb0 = CT(k.nose_b0_refl); t_na1 = CT(k.nose_a1_refl);
		t_nk = CT(k.nasal_k[5]);
	}
	auto stage_tube = [&](int c) {
		const unsigned long long t_stage = stamping ? clock64() : 0ull;
		// the section lane and the utterance: a DPP row of the row view, or the whole wavefront
		const int Lt = kTubePerWave ? lane : L;
		const int u = kTubePerWave ? sub : urow;
		const int valid = valid_in(u, c);
		const bool active = (kTubePerWave || U >= 4 || row < U) && (Lt < TL::kLanes);
		LaneSpec spec;
		{
			const int packed = kTubeHoist ? t_packed : reinterpret_cast<const int*>(sm.lanec + 72)[TL::kWaveWide ? (Lt < 48 ? Lt : 47) : (Lt & 15)];
			spec.link_right = static_cast<signed char>(packed & 7);
			spec.kl_slot = static_cast<signed char>(((packed >> 4) & 15) - 1);
			spec.kl_fixed = static_cast<signed char>((packed >> 8) & 15);
			spec.damp_left = static_cast<signed char>((packed >> 12) & 1);
			spec.inj_slot = static_cast<signed char>(((packed >> 16) & 15) - 1);
		}
		const CT* klp = sm.kl + at_kl(c & 1, u);
		const CT* injp = (kLaneRec ? sm.kl : sm.inj) + at_inj(c & 1, u);
		CT* oxp = sm.ox + (static_cast<size_t>(c & 1) * U + u) * C * 2;
		const bool is3l = (Lt == TL::kThreeWayRight) || (Lt == TL::kNasalFirst); // my left side is the 3-way junction
		const bool is3r = (Lt == TL::kThreeWayLeft);                            // my right side is the 3-way junction
		const bool ismouth = (Lt == TL::kMouth), isnose = (Lt == TL::kNose);
		const bool isend = ismouth || isnose;
		const CT damping = kTubeHoist ? t_damping : CT(k.damping);
		// every link of the 10+6 tube damps (uniform scalar); the 30+18 tube damps at region boundaries only
		const CT damp_l = (!TL::kWaveWide || spec.damp_left) ? damping : CT(1.0);
		const CT damp_r = (!TL::kWaveWide || spec.link_right != kCopy) ? damping : CT(1.0);
		const CT refl_b0 = ismouth ? (kTubeHoist ? t_mb0 : CT(k.mouth_b0_refl)) : (isnose ? (kTubeHoist ? t_nb0 : CT(k.nose_b0_refl)) : CT(0.0));
		const CT refl_a1 = ismouth ? (kTubeHoist ? t_ma1 : CT(k.mouth_a1_refl)) : (isnose ? (kTubeHoist ? t_na1 : CT(k.nose_a1_refl)) : CT(0.0));
		const CT kend_const = isnose ? (kTubeHoist ? t_nk : CT(k.nasal_k[5])) : CT(0.0); // nose aperture coefficient (fixed)
		const CT is_mouth = ismouth ? CT(1.0) : CT(0.0);
		// non-end lanes store their (meaningless) radiation input into the dump area
		CT* ox_w = (active && isend) ? oxp + (isnose ? C : 0) : sm.dump + 192 + lane; // [mouth | nose][C]
		const int ox_stride = (active && isend) ? 1 : 0;
		if constexpr (kBlockRec) {
#pragma clang fp contract(off)
			// Lane-indexed record in blocks of four steps (float, 10+6 tube): per block four 16-byte reads -- my left
			// coefficient, my right neighbour's, my 3-way / mouth coefficient, my injection, each for the block's four steps --
			// fetched one block ahead, and one 16-byte store of the four tops (a dump slot for the lanes that are not open ends).
			using V2 = float __attribute__((ext_vector_type(2)));
			using F4 = float __attribute__((ext_vector_type(4)));
			static_assert(C % 4 == 0 && 4 % D == 0, "blocks of four steps, a multiple of the section delay");
			const CT* const lds0 = reinterpret_cast<const CT*>(smem_raw);
			unsigned ik = static_cast<unsigned>(klp - lds0) + 4 * Lt; // {my left coefficient, my right neighbour's}: entries Lt, Lt + 1
			unsigned ic = static_cast<unsigned>(klp - lds0) + 4 * ((is3l || is3r) ? (Lt == TL::kNasalFirst ? kLrAu : kLrAlr) : (ismouth ? kLrK8 : (isnose ? kLrKn : kLrZero)));
			unsigned ii = static_cast<unsigned>(klp - lds0) + 4 * (spec.inj_slot >= 0 ? kLrInj + spec.inj_slot : kLrZero);
			asm volatile("" : "+v"(ik), "+v"(ic), "+v"(ii));
			const F4* pk = reinterpret_cast<const F4*>(lds0 + ik);
			const F4* pc = reinterpret_cast<const F4*>(lds0 + ic);
			const F4* pi = reinterpret_cast<const F4*>(lds0 + ii);
			F4* ox4 = (active && isend) ? reinterpret_cast<F4*>(oxp + (isnose ? C : 0)) : reinterpret_cast<F4*>(sm.dump) + lane;
			const int ox4_stride = (active && isend) ? 1 : 0;
			// One block of four steps (a macro: the loop below spells it out three times).  Per step:
			// - 3-way junction (VocalTractModel0.h:595-604): junctionPressure = aL * S4.top + aR * S5.bottom + aU * N1.bottom
			//   (alpha_left == alpha_right), each product rounded on the lane that owns the operand, summed left to right;
			// - open ends: reflection low-pass (ReflectionFilter.h:66-76) of k * top; an end lane's cc is its coefficient (the other
			//   lanes form a product nobody uses);
			// - the two links of a section as the halves of packed operations, every operation rounded on its own: top: x = "left
			//   top", y = my bottom, k = KL; bottom: x = "right bottom", y = my top, k = -KR; jm is what the 3-way junction sends
			//   towards S5 / N1 and back into S4; x + k d on top, x + (-KR) d == x - KR d on the bottom (the same rounded operations);
			// - T, B are the values written D steps ago; tops keeps the end lanes' top: the post-tube filters form the radiated
			//   part (1 + k) * top.
			// (the links as plain operations instead of the halves of packed ones -- no register pairs to assemble, twice the
			// arithmetic instructions, the same roundings -- where that measured faster: four utterances per workgroup at
			// SectionDelay 1, 4096 x 2 s 12.34 -> 12.03 ms; SectionDelay 2 the same either way, one utterance per workgroup 4 % slower)
			constexpr bool kPlainLinks = (U == 4 && D == 1);
#define GVTM_TUBE_LINKS \
					if constexpr (kPlainLinks) { \
						const CT ry = rmul(refl_b0, kT) - rmul(refl_a1, refl_y1); \
						refl_y1 = ry; \
						const CT tle = is3l ? (jp - B) : Tl; \
						CT bre = is3r ? (jp - T) : Br; \
						bre = isend ? ry : bre; \
						const CT pt = rmul(kl, tle - B), pb = rmul(kr, bre - T); \
						top[ph] = rmul(tle + pt, damp_l) + inj; \
						bot[ph] = rmul(bre - pb, damp_r) + CT(0.0); \
					} else { \
						const V2 rp = V2{refl_b0, refl_a1} * V2{kT, refl_y1}; \
						const CT ry = rp.x - rp.y; \
						refl_y1 = ry; \
						const V2 Y = {B, T}; \
						const V2 jm = V2{jp, jp} - Y; \
						const CT tle = is3l ? jm.x : Tl; \
						CT bre = is3r ? jm.y : Br; \
						bre = isend ? ry : bre; \
						const V2 X = {tle, bre}; \
						const V2 P = V2{kl, kr} * (X - Y); \
						const V2 N = V2{X.x + P.x, X.y - P.y} * V2{damp_l, damp_r} + V2{inj, CT(0.0)}; \
						top[ph] = N.x; \
						bot[ph] = N.y; \
					}
#define GVTM_TUBE_BLOCK(b_kl, b_kr, b_cc, b_inj) { \
				F4 tops; \
				_Pragma("unroll") \
				for (int q = 0; q < 4; ++q) { \
					const int ph = q % D; \
					const CT kl = b_kl[q], kr = b_kr[q], cc = b_cc[q], inj = b_inj[q]; \
					const CT T = top[ph], B = bot[ph]; \
					const CT Tl = from_left(T), Br = from_right(B); \
					const CT v = rmul(cc, is3r ? T : B); \
					const CT jp = (row_bcast<TL::kThreeWayLeft>(v) + row_bcast<TL::kThreeWayRight>(v)) + row_bcast<TL::kNasalFirst>(v); \
					const CT kT = rmul(cc, T); \
					GVTM_TUBE_LINKS \
					tops[q] = T; \
				} \
				*ox4 = tops; \
				ox4 += ox4_stride; \
			}
			F4 n_kl = pk[0], n_kr = pk[1], n_cc = pc[0], n_inj = pi[0];
			const unsigned long long t_loop = stamping ? clock64() : 0ull;
			if (stamping) sm.diag[6] += t_loop - t_stage;
			{
				// Two blocks per iteration, each with a register set of its own for its records (one is computed on while the other
				// is in flight): with one block per iteration the compiler copies the sixteen prefetched values into the working set
				// every block (eight 64-bit moves per four steps).  Same box, 4096 / 512 / 256 utterances: with one and two
				// utterances per workgroup, whose tick is the tube, 256 x 2 s 2.61 -> 2.44 ms; with four it was a loss while the
				// helpers were the tick (SectionDelay 2 x 2000 frames 97.7 -> 99.1 ms) and pays since the tube is the tick again
				// (93.0 -> 91.6 ms, SectionDelay 1 x 500 12.63 -> 12.42, SectionDelay 4 unchanged).
				int s0 = 0;
				for (; s0 + 4 < valid; s0 += 8) {
					pk += kKlLen; pc += kKlLen; pi += kKlLen;
					const F4 m_kl = pk[0], m_kr = pk[1], m_cc = pc[0], m_inj = pi[0];
					GVTM_TUBE_BLOCK(n_kl, n_kr, n_cc, n_inj)
					pk += kKlLen; pc += kKlLen; pi += kKlLen; // (one block past the chunk after its last pair: never consumed)
					n_kl = pk[0]; n_kr = pk[1]; n_cc = pc[0]; n_inj = pi[0];
					GVTM_TUBE_BLOCK(m_kl, m_kr, m_cc, m_inj)
				}
				// an odd number of blocks (a stream's launch keeps the state: not one step more than asked for)
				if (s0 < valid) GVTM_TUBE_BLOCK(n_kl, n_kr, n_cc, n_inj)
			}
#undef GVTM_TUBE_BLOCK
#undef GVTM_TUBE_LINKS
			if (stamping) sm.diag[7] += clock64() - t_loop;
			return;
		}
		if constexpr (kLaneRec) {
#pragma clang fp contract(off)
			// Lane-indexed record (float, 10+6 tube): three read cursors with the same constant stride.
			using V2 = float __attribute__((ext_vector_type(2)));
			constexpr int R = (D == 3) ? 6 : 4;
			static_assert(C % R == 0, "chunk must be a multiple of the tube unroll");
			// (the cursors as opaque element indices into the whole LDS block: seen as "region offset + lane", the compiler
			// folds a step's record offset into the region's and, the sum not fitting an immediate, adds it per read)
			const CT* const lds0 = reinterpret_cast<const CT*>(smem_raw);
			unsigned ik = static_cast<unsigned>(klp - lds0) + Lt; // {my left coefficient, my right neighbour's}
			unsigned ic = static_cast<unsigned>(klp - lds0) + ((is3l || is3r) ? (Lt == TL::kNasalFirst ? kLrAu : kLrAlr) : (ismouth ? kLrK8 : (isnose ? kLrKn : kLrZero)));
			unsigned ii = static_cast<unsigned>(klp - lds0) + (spec.inj_slot >= 0 ? kLrInj + spec.inj_slot : kLrZero);
			asm volatile("" : "+v"(ik), "+v"(ic), "+v"(ii));
			const CT* pk = lds0 + ik;
			const CT* pc = lds0 + ic;
			const CT* pi = lds0 + ii;
			CT* ox_c = ox_w;
			// records are fetched TWO steps ahead of their use; two register sets alternate by step parity
			CT n_kl = pk[0], n_kr = pk[1], n_cc = pc[0], n_inj = pi[0];
			pk += kKlLen; pc += kKlLen; pi += kInjLen;
			CT m_kl = pk[0], m_kr = pk[1], m_cc = pc[0], m_inj = pi[0];
			const unsigned long long t_loop = stamping ? clock64() : 0ull;
			if (stamping) sm.diag[6] += t_loop - t_stage;
			for (int s0 = 0; s0 < valid; s0 += R) {
#pragma unroll
				for (int q = 0; q < R; ++q) {
					const int ph = q % D;
					const CT kl = n_kl, kr = n_kr, cc = n_cc, inj = n_inj;
					n_kl = m_kl; n_kr = m_kr; n_cc = m_cc; n_inj = m_inj;
					pk += kKlLen; pc += kKlLen; pi += kInjLen; // (two records past the chunk after its last step: never consumed)
					m_kl = pk[0]; m_kr = pk[1]; m_cc = pc[0]; m_inj = pi[0];
					const CT T = top[ph], B = bot[ph]; // values written D steps ago
					const CT Tl = from_left(T), Br = from_right(B);
					// 3-way junction (VocalTractModel0.h:595-604): junctionPressure = aL * S4.top + aR * S5.bottom + aU * N1.bottom
					// (alpha_left == alpha_right), each product rounded on the lane that owns the operand, summed left to right
					const CT v = rmul(cc, is3r ? T : B);
					const CT jp = (row_bcast<TL::kThreeWayLeft>(v) + row_bcast<TL::kThreeWayRight>(v)) + row_bcast<TL::kNasalFirst>(v);
					// open ends: reflection low-pass (ReflectionFilter.h:66-76) of k * top; an end lane's cc is its coefficient (the
					// other lanes form a product nobody uses)
					const CT kT = rmul(cc, T);
					const V2 rp = V2{refl_b0, refl_a1} * V2{kT, refl_y1};
					const CT ry = rp.x - rp.y;
					refl_y1 = ry;
					// the two links of a section as the halves of packed operations, every operation rounded on its own:
					// top: x = "left top", y = my bottom, k = KL; bottom: x = "right bottom", y = my top, k = -KR
					const V2 Y = {B, T};
					const V2 jm = V2{jp, jp} - Y; // what the 3-way junction sends towards S5 / N1 and back into S4
					const CT tle = is3l ? jm.x : Tl;
					CT bre = is3r ? jm.y : Br;
					bre = isend ? ry : bre;
					const V2 X = {tle, bre};
					const V2 P = V2{kl, kr} * (X - Y);
					// x + k d on top, x + (-KR) d == x - KR d on the bottom (the same rounded operations)
					const V2 N = V2{X.x + P.x, X.y - P.y} * V2{damp_l, damp_r} + V2{inj, CT(0.0)};
					top[ph] = N.x;
					bot[ph] = N.y;
					*ox_c = T; // the end lanes' top: the post-tube filters form the radiated part (1 + k) * top
					ox_c += ox_stride;
				}
			}
			if (stamping) sm.diag[7] += clock64() - t_loop;
			return;
		}
		// my left junction coefficient: a record slot that changes every step, or a per-lane constant
		// parked in LDS (stride 0) so that the loop body is the same load for every lane
		const CT* kl_r = spec.kl_slot >= 0 ? klp + spec.kl_slot : sm.lanec + lane;
		const int kl_stride = spec.kl_slot >= 0 ? kKlLen : 0;
		const CT* inj_r = spec.inj_slot >= 0 ? injp + spec.inj_slot : sm.lanec + 64; // lanec[64] == 0
		const int inj_stride = spec.inj_slot >= 0 ? kInjLen : 0;

		// the record of the next step is fetched while the current one is computed; two register
		// sets alternate by step parity so that no copies are needed
		constexpr int R = (D == 3) ? 6 : 4;
		CT n_kl, n_inj, n_alr, n_au, n_k8, m_kl, m_inj, m_alr, m_au, m_k8;
		static_assert(C % R == 0, "chunk must be a multiple of the tube unroll");
		CT* ox_c = ox_w;
		const CT* pk = kl_r;
		const CT* pi = inj_r;
		const CT* pr = klp;
		// records are fetched TWO steps ahead of their use: wherever the scheduler places the loads inside a
		// step, they have a whole step to land (batch 4096 in float: 18.7 -> 17.6 ms against one step ahead)
		n_kl = *pk; n_inj = *pi; n_alr = pr[kKlAlr]; n_au = pr[kKlAu]; n_k8 = pr[kKlK8];
		pk += kl_stride; pi += inj_stride; pr += kKlLen;
		m_kl = *pk; m_inj = *pi; m_alr = pr[kKlAlr]; m_au = pr[kKlAu]; m_k8 = pr[kKlK8];
		// whole blocks of R steps: a partial last block runs on over stale records (the state is
		// never used after the utterance's last chunk)
		const unsigned long long t_loop = stamping ? clock64() : 0ull;
		if (stamping) sm.diag[6] += t_loop - t_stage;
		for (int s0 = 0; s0 < valid; s0 += R) {
#pragma unroll
			for (int q = 0; q < R; ++q) {
				{
					const int ph = q % D;
					const CT kl = n_kl, inj = n_inj, alr = n_alr, au = n_au, k8 = n_k8;
					n_kl = m_kl; n_inj = m_inj; n_alr = m_alr; n_au = m_au; n_k8 = m_k8;
					{
						// advance the three read cursors (after the chunk's last step they point two records
						// past it; those prefetches are never consumed)
						pk += kl_stride; pi += inj_stride; pr += kKlLen;
						m_kl = *pk; m_alr = pr[kKlAlr]; m_au = pr[kKlAu]; m_k8 = pr[kKlK8];
						m_inj = *pi;
					}
					const CT T = top[ph], B = bot[ph]; // values written D steps ago
					CT Tl, Br, kr;
					if constexpr (TL::kWaveWide) {
						Tl = from_left_wave(T); Br = from_right_wave(B); kr = from_right_wave(kl);
					} else {
						Tl = from_left(T); Br = from_right(B); kr = from_right(kl);
					}
					// 3-way junction (VocalTractModel0.h:595-604): alpha_left == alpha_right
					// junctionPressure = aL * S4.top + aR * S5.bottom + aU * N1.bottom, the three products rounded
					// and summed left to right as the reference does
					CT jp;
					if constexpr (TL::kWaveWide) {
						jp = rmul(alr, lane_value<TL::kThreeWayLeft>(T)) + rmul(alr, lane_value<TL::kThreeWayRight>(B)) +
								rmul(au, lane_value<TL::kNasalFirst>(B));
					} else {
						// every lane of a row gets its own utterance's three operands by row broadcast
						jp = rmul(alr, row_bcast<TL::kThreeWayLeft>(T)) + rmul(alr, row_bcast<TL::kThreeWayRight>(B)) +
								rmul(au, row_bcast<TL::kNasalFirst>(B));
					}
					CT tn, bn, kend, kT;
					if constexpr (sizeof(CT) == 4) {
#pragma clang fp contract(off)
						// Float: the two links of a section have the same shape, x + k (x - y) scaled by the damping --
						// top: x = "left top", y = my bottom, k = KL; bottom: x = "right bottom", y = my top, k = -KR
						// (the sign is exact) -- so they run as the two halves of packed instructions, every
						// operation still rounded on its own (v_pk_add_f32 / v_pk_mul_f32, no fused multiply-add).
						using V2 = float __attribute__((ext_vector_type(2)));
						kend = is_mouth * k8 + kend_const;
						kT = rmul(kend, T);
						const V2 rp = V2{refl_b0, refl_a1} * V2{kT, refl_y1}; // ReflectionFilter.h:66-76
						const CT ry = rp.x - rp.y;
						refl_y1 = ry;
						const V2 Y = {B, T};
						const V2 jm = V2{jp, jp} - Y; // what the 3-way junction sends towards S5 / N1 and back into S4
						const CT tle = is3l ? jm.x : Tl;
						CT bre = is3r ? jm.y : Br;
						bre = isend ? ry : bre;
						const V2 X = {tle, bre};
						const V2 P = V2{kl, -kr} * (X - Y);
						const V2 N = (X + P) * V2{damp_l, damp_r} + V2{inj, CT(0.0)};
						tn = N.x;
						bn = N.y;
					} else {
						// left link -> my new top.  3-way lanes: KL is 0 and the "left top" is jp - B, which
						// gives (jp - B) * damping + inj exactly; copies: KL 0, damp 1, inj 0 give Tl exactly.
						const CT tle = is3l ? (jp - B) : Tl;
						const CT dl = rmul(kl, tle - B);
						tn = rmul(tle + dl, damp_l) + inj;
						// open ends: reflection low-pass (ReflectionFilter.h:66-76) of k * top
						kend = is_mouth * k8 + kend_const;
						kT = rmul(kend, T);
						const CT ry = rmul(refl_b0, kT) - rmul(refl_a1, refl_y1);
						refl_y1 = ry;
						// right link -> my new bottom.  KR (my right neighbour's KL) is 0 for copies, delays,
						// the 3-way and the ends, whose "right bottom" is jp - T resp. the reflected wave.
						const CT jt = jp - T;
						CT bre = is3r ? jt : Br;
						bre = isend ? ry : bre;
						const CT dr = rmul(kr, T - bre);
						bn = rmul(bre + dr, damp_r); // feeds next step's differences: rounded here
					}
					top[ph] = tn;
					bot[ph] = bn;
					// radiated part, filtered later by F2: (1 + k) * top at mouth and nose
					const CT rad_in = (CT(1.0) + kend) * T;
					*ox_c = rad_in;
					ox_c += ox_stride;
				}
			}
		}
		if (stamping) sm.diag[7] += clock64() - t_loop;
	};

	// -------------------------------------------------------------------------------------
	// the tick loop

	// Issue priority on the shared SIMDs.  In fp64 the tube wavefront is the longest chain by a margin and
	// gains from outranking the other serial roles (4.35 -> 4.13 ms on batch 256); in float the roles are
	// balanced and a flat priority measured best (3.86 vs 3.99 ms).
	if constexpr (sizeof(CT) == 8) {
		if (role == 0) __builtin_amdgcn_s_setprio(3);
		else if (role < 5) __builtin_amdgcn_s_setprio(1);
	} else {
		if (role < 5) __builtin_amdgcn_s_setprio(2);
	}

	const int n_ticks = max_chunks + 6;
	// output samples a chunk can produce (the last one also converts the 2*pad flush zeros), in 64-lane passes
	const int p6_passes = kP6Groups * static_cast<int>(((static_cast<uint64_t>(C + 2 * k.pad) << 16) / k.time_inc + 2 + 63 + 63) / 64);
	// the tube and the pre-tube filter wavefronts run tick loops of their own (same trip count, one barrier per tick like
	// everybody else): only their own state is live in them, so the register allocator does not spill around the helper
	// passes' code into their prologues
	if (role == 0) {
		for (int t = -2; t < n_ticks; ++t) {
			const unsigned long long t_begin = stamping ? clock64() : 0ull;
			TR(t, 1);
			if (!(GVTM_TUNE_SKIP & 64)) stage_tube(t - 4);
			TR(t, 2);
			if (stamping) role_busy += clock64() - t_begin;
			__syncthreads();
		}
	} else if (role == 2) {
		for (int t = -2; t < n_ticks; ++t) {
			const unsigned long long t_begin = stamping ? clock64() : 0ull;
			TR(t, 1);
			if (!(GVTM_TUNE_SKIP & 256)) stage_f1(t - 3);
			TR(t, 2);
			if (stamping) role_busy += clock64() - t_begin;
			__syncthreads();
		}
	} else
	for (int t = -2; t < n_ticks; ++t) {
		unsigned long long t_begin = 0;
		if (stamping) t_begin = clock64();
		auto live = [&](int c) { return c >= 0 && c < max_chunks; };
		// Helper wavefronts pull passes (one stage over up to 64 items) from the tick's list through
		// an LDS ticket counter, heaviest stages first, so that they finish together whatever NH is.
		auto help = [&]() {
			constexpr int kStepPasses = (U * C + 63) / 64;
			constexpr int kHalfPasses = (2 * U * C + 64 * kP4aItems - 1) / (64 * kP4aItems);
			const int n_passes = p6_passes + 4 * kStepPasses + kHalfPasses;
			// A helper wavefront's FIRST pass of a tick is its own by position (pass number = its index among the helpers, no
			// ticket: right after the barrier every helper asks at once and the first ticket costs ~1300 cycles); the rest of
			// the list, and everything the joining serial wavefronts take, goes by ticket (the counter starts behind them).
			// Where (kStaticRounds): same box, bench.py, 4096 utterances x 500 frames, without / with: float (eleven helpers)
			// SectionDelay 2 24.5 -> 23.6 ms (configs[3] 366.6 -> 352.8), 3: 60.0 -> 58.6, 1 and 4 unchanged -- with seven helpers
			// it was SLOWER (108.2 -> 111.4 per 2000 frames); fp64 SectionDelay 1 21.5 -> 20.4 ms, SectionDelay 2 40.6 -> 39.5
			// (x 2000: 160.7 -> 156.3); mixed SectionDelay 1 19.8 -> 19.1, SectionDelay 2 36.4 -> 36.6 (off); double at SectionDelay
			// 3 and 4 unchanged (off); +3.5 % with two utterances per workgroup at SectionDelay 3 and on the 30 + 18 tube (off);
			// two or three rounds by position lose everywhere (profiles/r03_whatif_role_cycles.txt, DESIGN.md 6 A/B table).
			// (the two forms spelled out separately, down to the dead comparison: see kHelperByRole)
			[[maybe_unused]] int own_round;
			if constexpr (kHelperByRole) own_round = (role == 5) ? 0 : kStaticRounds;
			else own_round = (wave >= kFirstHelper) ? 0 : kStaticRounds;
			for (;;) {
				unsigned idx = 0;
				if constexpr (kHelperByRole) {
					if (own_round < kStaticRounds) {
						idx = static_cast<unsigned>(own_round * NH + (wave - kFirstHelper));
						++own_round;
					} else {
						if (lane == 0) idx = atomicAdd(&sm.ticket[t & 1], 1u);
						idx = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(idx)));
					}
				} else if constexpr (kStaticRounds > 0) {
					if (own_round < kStaticRounds) {
						idx = static_cast<unsigned>(own_round * NH + (wave - kFirstHelper));
						++own_round;
					} else {
						if (lane == 0) idx = atomicAdd(&sm.ticket[t & 1], 1u);
						idx = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(idx)));
					}
				} else {
					if (lane == 0) idx = atomicAdd(&sm.ticket[t & 1], 1u);
					idx = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(idx)));
				}
				if (idx >= static_cast<unsigned>(n_passes)) break; // (fewer passes than helpers: nothing is left for the ticketed rest either)
				int ps = static_cast<int>(idx);
				TR(t, 0x100u | idx);
				const unsigned long long d0_ = stamping ? clock64() : 0ull;
				int stage;
				// (GVTM_TUNE_SKIP: instruction-count experiments only -- a skipped stage leaves garbage behind)
				if (ps < p6_passes) {
					stage = 5;
					if (!(GVTM_TUNE_SKIP & 32) && live(t - 6)) stage_p6(t - 6, ps);
				} else if ((ps -= p6_passes) < kStepPasses) {
					stage = 4;
					if (!(GVTM_TUNE_SKIP & 16) && live(t - 2)) stage_p4b(t - 2, ps);
				} else if ((ps -= kStepPasses) < kStepPasses) {
					stage = 2;
					if (!(GVTM_TUNE_SKIP & 4) && live(t - 2)) stage_p2c(t - 2, ps);
				} else if ((ps -= kStepPasses) < kStepPasses) {
					stage = 1;
					if (!(GVTM_TUNE_SKIP & 2) && live(t - 3)) stage_p2b(t - 3, ps);
				} else if ((ps -= kStepPasses) < kStepPasses) {
					stage = 0;
					if (!(GVTM_TUNE_SKIP & 1) && live(t + 1)) stage_p2a(t + 1, ps);
				} else {
					stage = 3;
					ps -= kStepPasses;
					if (!(GVTM_TUNE_SKIP & 8) && live(t - 1)) stage_p4a(t - 1, ps);
				}
				if (stamping) atomicAdd(&sm.diag[stage], clock64() - d0_);
				TR(t, 0x200u | idx);
			}
		};
		TR(t, 1);
		switch (role) {
		case 0: stage_tube(t - 4); break;
		case 1: if (!(GVTM_TUNE_SKIP & 128)) stage_s1(t); break;
		case 2: stage_f1(t - 3); break;
		case 3: if (!(GVTM_TUNE_SKIP & 512)) stage_f2(t - 5); break;
		case 4: if (!(GVTM_TUNE_SKIP & 1024)) stage_interp(t); break;
		default:
			if (wave == kFirstHelper) {
				if (lane == 0) {
					if constexpr (kHelperByRole || kStaticRounds > 0) sm.ticket[(t + 1) & 1] = static_cast<unsigned>(kStaticRounds * NH); // next tick's counter (idle this tick)
					else sm.ticket[(t + 1) & 1] = 0u;
				}
				// (the resampler's output ranges for next tick.  When they were two emulated 64-bit divisions per utterance, moving
				// them to the interpolation or the pre-tube filter wavefront, which have time to spare, measured slower on configs[3]
				// in every precision: 108.2 -> 111.5 / 108.6 ms in float, 148.5 -> 159.3 / 150.6 mixed, 156.3 -> 163.5 / 159.4 fp64
				// per 2000 frames.  Where bounds_by_recurrence() says so they are carried from tick to tick now, in this
				// wavefront's registers.)
				if constexpr (U > 1) stage_bounds(t);
			}
			break;
		}
		// A serial wavefront whose stage is done early joins the helpers for the rest of the tick, at their priority.
		// (ONE call site for all of them: the passes are some 30 KB of code.)
		TR(t, 2);
		constexpr unsigned kHelpMask = kSerialHelpMask;
		constexpr bool kSerialHelp = !kTubePerWave && G == 1 && kHelpMask != 0;
		const bool joins = kSerialHelp && role < 5 && ((kHelpMask >> role) & 1) != 0;
		if (role == 5 || joins) {
			if (joins) {
				if (stamping) role_busy += clock64() - t_begin;
				__builtin_amdgcn_s_setprio(0);
			}
			help();
			if (joins) {
				if constexpr (sizeof(CT) == 8) __builtin_amdgcn_s_setprio(1);
				else __builtin_amdgcn_s_setprio(2);
				if (stamping) t_begin = clock64(); // its own busy time only
			}
		}
		if (stamping) role_busy += clock64() - t_begin;
		TR(t, 3);
		__syncthreads();
	}

	if constexpr (kTubePerWave) {
		// diagnostics: the first tube wavefront stands for all of them
		if (stamping && (role > 0 || wave == 0) && role + (wave - kSerial) < 8) a.phase_cycles[group * 16 + (role < 5 ? role : 5 + wave - kSerial)] = role_busy;
	} else {
		if (stamping && sub == 0 && (role < 5 || (role == 5 && wave - kFirstHelper < 3))) a.phase_cycles[group * 16 + (role < 5 ? role : 5 + wave - kFirstHelper)] = role_busy;
	}
	__syncthreads();
	if (a.phase_cycles != nullptr && tid < 8) a.phase_cycles[group * 16 + 8 + tid] = sm.diag[tid];

	// ---- SampleRateConverter's flush overrun (SampleRateConverter.h:298-308 with :462-471), down-sampling only.
	// When an automatic dataEmpty() has left the empty pointer beyond its end pointer and flushBuffer()'s final
	// dataEmpty() comes before the fills have caught up, the reference sees endPtr < emptyPtr_, adds BUFFER_SIZE and
	// converts one more lap of the ring: outputs whose read position lies in [emptyPtr, fills + 1024), computed from
	// whatever the 1024 slots hold at that moment (slot r = the newest fill of residue class r).  The ring here is
	// 1024 samples long for down-sampling plans and indexed by the sample number, so it aliases the same way: the
	// ordinary per-output evaluation over the final ring contents yields the reference's samples.
	if (!k.upsampling && kFinal) {
		for (int u = 0; u < U; ++u) {
			const Extent e = sm.ext[u];
			uint64_t k_from = 0, k_to = 0;
			if (e.nchunks == 0 || !src_flush_overrun(k.time_inc, k.pad, e.step_base + e.steps, k_from, k_to)) continue;
			const ST* xr = sm.x + u * XRS;
			float mx = 0.0f;
			for (uint64_t ko = k_from + tid; ko < k_to; ko += kThreads) {
				const uint64_t t = ko * k.time_inc;
				const int base = static_cast<int>(t >> 16) - k.pad;
				const unsigned frac = static_cast<unsigned>(t & 0xFFFFu);
				ST acc = ST(0);
				unsigned ph = static_cast<unsigned>(rint(static_cast<CT>(frac) * CT(k.src_ratio)));
				unsigned ii;
				int j = 0;
				while ((ii = (ph >> 8)) < static_cast<unsigned>(kSrcFilterLength)) {
					const SrcTap<ST> cf = src_tap(ii);
					const ST coef = mad(cf.dh, static_cast<ST>(ph & 0xFFu) / ST(256), cf.h);
					acc = mad(xr[(base - j) & (XR - 1)], coef, acc);
					++j;
					ph += k.phase_inc;
				}
				ph = static_cast<unsigned>(rint(static_cast<CT>((~frac) & 0xFFFFu) * CT(k.src_ratio)));
				j = 0;
				while ((ii = (ph >> 8)) < static_cast<unsigned>(kSrcFilterLength)) {
					const SrcTap<ST> cf = src_tap(ii);
					const ST coef = mad(cf.dh, static_cast<ST>(ph & 0xFFu) / ST(256), cf.h);
					acc = mad(xr[(base + 1 + j) & (XR - 1)], coef, acc);
					++j;
					ph += k.phase_inc;
				}
				const float y = static_cast<float>(acc);
				if (ko - e.k_first < a.audio_stride) a.audio[GVTM_ROW_UTT(u, (group * U + u)) * a.audio_stride + (ko - e.k_first)] = y;
				mx = fmaxf(mx, fabsf(y));
			}
			if (mx > 0.0f) atomicMax(&sm.peak[u], __float_as_uint(mx));
		}
	}

	// ---- per-utterance peak (for Util::calculateOutputScale) and sample count
	__syncthreads();
	if (tid < U) {
		const size_t ug = GVTM_ROW_UTT(tid, group * U + tid);
		if (ug < a.batch) {
			if (a.maxabs) a.maxabs[ug] = __uint_as_float(sm.peak[tid]);
			const Extent e = sm.ext[tid];
			const uint64_t total = e.step_base + e.steps;
			const uint64_t k_end = kFinal ? src_output_count(k.time_inc, k.pad, k.upsampling, total) : ((total << 16) + k.time_inc - 1) / k.time_inc;
			if (a.out_counts) a.out_counts[ug] = static_cast<int64_t>(k_end - e.k_first);
		}
	}

	// ---- a stream's states for the next launch
	if (a.stream) {
		if constexpr (TARGETS) {
			// the moving averages' sums, push and finish alike (a push synthesizes whole blocks of four steps: no lane ran on)
			if (role == 4 && rowp < U && sm.ext[rowp].frames > 0) {
				double* sums = reinterpret_cast<double*>(a.stream + GVTM_ROW_UTT(rowp, (group * U + rowp)) * a.stream_stride + SL::sums(kTubeLanes, kTubeWords, XR));
				sums[Lp] = tg.sum;
			}
		}
		if (serial_live && (kTubePerWave && role == 0 ? true : (U >= 4 || row < U))) {
			unsigned char* sb = a.stream + GVTM_ROW_UTT(serial_utt, (group * U + serial_utt)) * a.stream_stride;
			CT* sc = reinterpret_cast<CT*>(sb + SL::scalars());
			if (role == 1 && L == 0) {
				sc[kSsPos] = sc_pos;
				sc[kSsPrev] = sc_prev;
				reinterpret_cast<StreamHeader*>(sb)->seed = sc_seed;
			} else if (role == 2 && (lane & 15) == 0 && (kRowView || lane < 16)) {
				sc[kSsBp] = bp_x1; sc[kSsBp + 1] = bp_x2; sc[kSsBp + 2] = bp_y1; sc[kSsBp + 3] = bp_y2;
				sc[kSsThr] = thr_y1;
			} else if (role == 3 && L < 2) {
				const int w2 = (L == 0) ? kSsRadMouth : kSsRadNose;
				sc[w2] = rad_x1;
				sc[w2 + 1] = rad_y1;
			} else if (role == 0) {
				const int Lt = kTubePerWave ? lane : L;
				if (Lt < kTubeLanes) {
					CT* tb = reinterpret_cast<CT*>(sb + SL::tube()) + Lt * kTubeWords;
#pragma unroll
					for (int i = 0; i < kTubeWords; ++i) tb[i] = st[i];
				}
			}
		}
		for (int u = 0; u < U; ++u) {
			if (GVTM_ROW_UTT(u, group * U + u) >= a.batch) break;
			const Extent e = sm.ext[u];
			unsigned char* sb = a.stream + GVTM_ROW_UTT(u, (group * U + u)) * a.stream_stride;
			ST* ring = reinterpret_cast<ST*>(sb + SL::ring(kTubeLanes, kTubeWords));
			for (int i = tid; i < XR; i += kThreads) ring[i] = sm.x[u * XRS + i];
			// the decimator's pre-roll for the next step: the 48 oversampled source values in front of it, which end
			// the last chunk's slot (its own pre-roll included when the chunk was short)
			const int lc = e.nchunks - 1;
			const int valid_last = static_cast<int>(e.steps) - lc * C;
			const CT* wsl = sm.w + (static_cast<size_t>(lc % 3) * U + u) * (kWPre + 2 * C) + 2 * valid_last;
			CT* pre = reinterpret_cast<CT*>(sb + SL::wpre(kTubeLanes, kTubeWords));
			for (int i = tid; i < kWPre; i += kThreads) pre[i] = wsl[i];
			if (tid == 0) {
				StreamHeader* h = reinterpret_cast<StreamHeader*>(sb);
				h->step_base = e.step_base + e.steps;
				h->peak_bits = sm.peak[u];
			}
		}
	}
}

#undef GVTM_ROW_UTT
#undef GVTM_KF

} // namespace v2
