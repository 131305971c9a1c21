// Event lists from posture sequences on the device (vtm_rules.hpp; EventList.cpp:302-371, 373-432, 435-676).
//
// What the reference's list comes to (vtm_rules.hpp): a map from event time to 32 values in which the later
// insertEvent call at a (time, parameter) wins.  A rule application k with start z_k and (int)duration d_k makes times
// q(z_k) + j * cp for the slots j = 0 .. W_k + 1, W_k = (q(z_k + d_k) - q(z_k)) / cp >= 1 and q(t) = t - t % cp.  The slots
// below W_k are the rule's WINDOW: no later rule reaches them.  The slots W_k and W_k + 1 lie in the windows that follow,
// as their slots 0 and 1, and go there as a CARRY: two presence bits and, per parameter, two values, over which the
// calls of the later rule win.  (With W_{k+1} = 1 the second carried slot is carried on once more.)
//
// Three kernels, no scratch; one wavefront per utterance in the first and the last:
//   count  the walk -- rule by rule: the match (a lane per rule, one ballot), the rule's symbols (rules_begin, the same in
//          every lane), then per window a bitmap of the slots some call reaches: the lanes 0-15 walk the 16 regular
//          profiles, 16-31 the special ones, lane 32 the markers (rules_profile / rules_markers with a functor that sets a
//          bit).  The window's events are the set bits below W_k.  Leaves the list's length, the status, the rule data and
//          the onsets.
//   scan   lengths to offsets (vtm_offsets_scan.hpp); a list that does not fit is dropped with status 5.
//   write  the walk again (nothing is kept between the kernels but the offsets); per window the events are staged in LDS,
//          32 at a time: +infinity everywhere, the times from the bitmap, the carried values, then the profiles once more
//          with a functor that stores at the rank of its slot -- a lane's calls run in the reference's order, so its later
//          store wins -- and the stage leaves as 8-byte units, 37 per event, 64 consecutive units per store instruction.
// Bit parity with the host: rules_begin, rules_profile and rules_event_time are the host's text; no FMA contraction.
#include "vtm_rules.hpp"
#include "vtm_offsets_scan.hpp"

namespace gvtm {

namespace {

static_assert(sizeof(gvtm_event) == 296 && sizeof(gvtm_event) % 8 == 0 && offsetof(gvtm_event, interp) == 8 && offsetof(gvtm_event, param) == 40 &&
		offsetof(gvtm_event, special) == 40 + 8 * kRulesParams,
		"an event is 37 units of 8 bytes: time / has_interp, interp[4], param[16], special[16]");
constexpr int kUnits = sizeof(gvtm_event) / 8;
constexpr int kValueUnit = 5;  // unit of param[0]; lane s < 32 owns unit kValueUnit + s
constexpr unsigned long long kInfinityBits = 0x7ff0000000000000ull; // Event::EMPTY_PARAMETER
constexpr int kWindowWords = 64;                  // one 64-bit word of the window's bitmap per lane
constexpr int kWindowSlots = kWindowWords * 64;   // W + 2 slots must fit: a rule of up to 4094 control periods
constexpr int kStageEvents = 32;                  // events staged in LDS at a time

__device__ __forceinline__ unsigned long long bits_below(int n) // n in [0, 64]
{
	return n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

// the LDS of one utterance's wavefront
struct Shared {
	float sym[kRulesSymbols];
	unsigned int bitmap32[2 * kWindowWords]; // atomicOr works on 32-bit words; word w of the 64-bit view is [2w], [2w + 1]
	unsigned long long present[kWindowWords]; // the bitmap with the carried bits or'ed in
	int prefix[kWindowWords];                 // events of the window in front of word w
	unsigned long long stage[kStageEvents * kUnits];
};

// a call reaches slot (q - q0) / cp of the window: the counting pass sets its bit
struct SlotBits {
	Shared& sh;
	const RuleApplication& a;
	int cp, q0, n_slots;
	bool bad = false;
	__device__ void at(double time)
	{
		int q;
		const int how = rules_event_time(time, a.zero_ref, a.dur_int, cp, q);
		if (how < 0) bad = true;
		if (how <= 0) return;
		const int j = (q - q0) / cp;
		if (j >= 0 && j < n_slots) atomicOr(&sh.bitmap32[j >> 5], 1u << (j & 31));
	}
	__device__ void operator()(double time, double) { at(time); }
	__device__ void operator()(double time) { at(time); }
};

// ... and the writing pass stores the value: into the stage at the slot's rank, or into the carry
struct SlotStore {
	Shared& sh;
	const RuleApplication& a;
	int cp, q0, window; // window: W
	int tile_first, tile_count, unit;
	double carry[2];
	bool carried[2];
	__device__ int rank(int j) const { return sh.prefix[j >> 6] + __popcll(sh.present[j >> 6] & bits_below(j & 63)); }
	__device__ void put(int j, double value)
	{
		if (j < window) {
			const int r = rank(j) - tile_first;
			if (r >= 0 && r < tile_count) sh.stage[r * kUnits + unit] = static_cast<unsigned long long>(__double_as_longlong(value));
		} else if (j == window) { // (not indexed: the four stay in registers)
			carry[0] = value;
			carried[0] = true;
		} else if (j == window + 1) {
			carry[1] = value;
			carried[1] = true;
		}
	}
	__device__ void operator()(double time, double value)
	{
		int q;
		if (rules_event_time(time, a.zero_ref, a.dur_int, cp, q) <= 0) return;
		const int j = (q - q0) / cp;
		if (j >= 0) put(j, value);
	}
};

__device__ __forceinline__ int quantise(int t, int cp)
{
	return cp != 1 ? t - t % cp : t;
}

// One utterance, one wavefront, all 64 lanes active.  kWrite false: the counting pass; true: the writing pass, which
// trusts the offsets (a list of no events returns at once) and guards every store by the list's room.
template <bool kWrite>
__device__ __forceinline__ void run_utterance(const RulesArgs& a, size_t utt, int lane, Shared& sh)
{
#pragma clang fp contract(off)
	const gvtm_rules_model& m = a.m;
	const int cp = a.control_period;
	const int64_t first_posture = a.posture_offsets[utt];
	const int64_t n64 = a.posture_offsets[utt + 1] - first_posture;
	unsigned long long* dst = nullptr;
	int64_t room = 0; // units of the list
	if (kWrite) {
		const int64_t out_first = a.event_offsets_out[utt], out_end = a.event_offsets_out[utt + 1];
		if (out_first < 0 || out_end > a.out_capacity || out_end <= out_first) return;
		dst = reinterpret_cast<unsigned long long*>(a.events_out + out_first);
		room = (out_end - out_first) * kUnits;
	}
	int32_t status = kRulesOk;
	if (n64 < 2 || n64 > 0x7fffffff) status = kRulesBadPosture;
	const int n = status == kRulesOk ? static_cast<int>(n64) : 0;
	const gvtm_posture* postures = a.postures + first_posture;
	if (status == kRulesOk) {
		bool bad = false;
		for (int i = lane; i < n; i += 64) bad = bad || postures[i].posture < 0 || postures[i].posture >= m.n_postures;
		if (__ballot(bad)) status = kRulesBadPosture;
	}
	if (!kWrite && lane == 0 && a.onsets && n64 > 0) a.onsets[first_posture] = 0.0;

	int64_t count = 0;   // events of the windows passed
	int n_rules = 0;
	int zero_ref = 0;
	int carry_present = 0;                 // bits 0 and 1: the slots 0 and 1 of the coming window hold an event
	double carry[2] = {0.0, 0.0};          // writing pass, lane s < 32: the values carried into those slots
	bool carried[2] = {false, false};
	int base = 0;
	while (status == kRulesOk && base < n - 1) {
		const gvtm_posture* p = postures + base;
		const int n_avail = n - base < 4 ? n - base : 4;
		int rule = -1;
		for (int r0 = 0; r0 < m.n_rules && rule < 0; r0 += 64) {
			const unsigned long long hits = __ballot(r0 + lane < m.n_rules && rules_match(m, r0 + lane, p, n_avail));
			if (hits) rule = r0 + __ffsll(static_cast<long long>(hits)) - 1;
		}
		if (rule < 0) {
			status = kRulesNoRule;
			break;
		}
		__syncthreads(); // the window before has been read
		// (every lane evaluates the same rule symbols and leaves the same float symbols in LDS, where the profiles read them)
		RuleApplication app;
		rules_begin(m, rule, p, n_avail, zero_ref, cp, sh.sym, app);
		if (app.status != kRulesOk) {
			status = app.status;
			break;
		}
		const int q0 = quantise(zero_ref, cp);
		const int next_zero = zero_ref + app.dur_int;
		const int window = (quantise(next_zero, cp) - q0) / cp; // >= 1: dur_int >= cp + 1
		const int n_slots = window + 2;
		if (window < 1 || n_slots > kWindowSlots) {
			status = kRulesNoRoom;
			break;
		}
		sh.bitmap32[lane] = 0;
		sh.bitmap32[lane + 64] = 0;
		__syncthreads();
		if (!kWrite && lane == 0) {
			if (a.rule_data && n_rules < a.max_rules) {
				a.rule_data[utt * static_cast<size_t>(a.max_rules) + n_rules] =
						gvtm_rule_data{rule + 1, base, base + app.n_expr - 1, zero_ref, app.mark1, app.mark2, app.duration, app.beat + zero_ref};
			}
			if (a.onsets) {
				for (int k = 1; k < app.n_expr; ++k) a.onsets[first_posture + base + k] = zero_ref + app.beat;
			}
		}
		++n_rules;
		{
			SlotBits bits{sh, app, cp, q0, n_slots};
			if (lane < 2 * kRulesParams) {
				rules_profile(m, app, p, sh.sym, lane & (kRulesParams - 1), lane >= kRulesParams, bits);
			} else if (lane == 2 * kRulesParams) {
				rules_markers(app, bits);
				atomicOr(&sh.bitmap32[window >> 5], 1u << (window & 31)); // the closing marker, at the next rule's start
			}
			if (__ballot(bits.bad)) {
				status = kRulesBadValue;
				break;
			}
		}
		__syncthreads();
		// the window's events: its bits below W, with the carried ones
		unsigned long long word = static_cast<unsigned long long>(sh.bitmap32[2 * lane]) | static_cast<unsigned long long>(sh.bitmap32[2 * lane + 1]) << 32;
		if (lane == 0) word |= static_cast<unsigned long long>(carry_present);
		const int below = window - 64 * lane; // slots of my word that lie in the window
		const unsigned long long mine = word & bits_below(below < 0 ? 0 : below > 64 ? 64 : below);
		int sum = __popcll(mine); // inclusive sums over the lanes
		for (int step = 1; step < 64; step <<= 1) {
			const int other = __shfl_up(sum, step);
			if (lane >= step) sum += other;
		}
		const int in_window = __shfl(sum, 63);
		sh.present[lane] = word;
		sh.prefix[lane] = sum - __popcll(mine);
		__syncthreads();
		// what this rule and the carry leave in the two slots behind the window
		int next_present = 0;
		for (int c = 0; c < 2; ++c) {
			const int j = window + c;
			if ((sh.present[j >> 6] >> (j & 63)) & 1ull) next_present |= 1 << c;
		}
		if (kWrite) {
			SlotStore store{sh, app, cp, q0, window, 0, 0, kValueUnit + lane, {0.0, 0.0}, {false, false}};
			for (int tile = 0; tile < in_window; tile += kStageEvents) {
				const int tile_count = in_window - tile < kStageEvents ? in_window - tile : kStageEvents;
				for (int u = lane; u < tile_count * kUnits; u += 64) sh.stage[u] = u % kUnits < kValueUnit ? 0ull : kInfinityBits;
				__syncthreads();
				// the times: the set bits of my word, at their ranks
				int r = sh.prefix[lane] - tile;
				for (unsigned long long w = mine; w; w &= w - 1, ++r) {
					if (r >= 0 && r < tile_count) {
						const unsigned time = static_cast<unsigned>(q0 + (64 * lane + __ffsll(static_cast<long long>(w)) - 1) * cp);
						sh.stage[r * kUnits] = static_cast<unsigned long long>(time); // has_interp = 0 above it
					}
				}
				if (lane < 2 * kRulesParams) {
					store.tile_first = tile;
					store.tile_count = tile_count;
					store.carry[0] = store.carry[1] = 0.0;
					store.carried[0] = store.carried[1] = false;
					// the values carried in first: this rule's calls win over them
					if (carried[0]) store.put(0, carry[0]);
					if (carried[1]) store.put(1, carry[1]);
					rules_profile(m, app, p, sh.sym, lane & (kRulesParams - 1), lane >= kRulesParams, store);
				}
				__syncthreads();
				const int64_t at = (count + tile) * kUnits;
				for (int u = lane; u < tile_count * kUnits; u += 64) {
					if (at + u < room) dst[at + u] = sh.stage[u];
				}
				__syncthreads();
			}
			carry[0] = store.carry[0];
			carry[1] = store.carry[1];
			carried[0] = store.carried[0];
			carried[1] = store.carried[1];
		}
		count += in_window;
		carry_present = next_present;
		zero_ref = next_zero;
		base += app.n_expr - 1;
	}

	// behind the last rule: its closing event and what may lie one period behind that
	const int tail = status == kRulesOk ? 1 + ((carry_present >> 1) & 1) : 0;
	if (!kWrite) {
		if (lane == 0) {
			a.event_offsets_out[utt + 1] = status == kRulesOk ? count + tail : 0;
			if (a.status) a.status[utt] = status;
			if (a.rule_counts) a.rule_counts[utt] = status == kRulesOk ? n_rules : 0;
		}
		return;
	}
	if (status != kRulesOk) return;
	__syncthreads();
	const int q_end = quantise(zero_ref, cp);
	for (int u = lane; u < tail * kUnits; u += 64) {
		const int c = u % kUnits;
		sh.stage[u] = c == 0 ? static_cast<unsigned long long>(static_cast<unsigned>(q_end + (u / kUnits) * cp)) : c < kValueUnit ? 0ull : kInfinityBits;
	}
	__syncthreads();
	if (lane < 2 * kRulesParams) {
		for (int c = 0; c < tail; ++c) {
			if (carried[c]) sh.stage[c * kUnits + kValueUnit + lane] = static_cast<unsigned long long>(__double_as_longlong(carry[c]));
		}
	}
	__syncthreads();
	for (int u = lane; u < tail * kUnits; u += 64) {
		if (count * kUnits + u < room) dst[count * kUnits + u] = sh.stage[u];
	}
}

__global__ __launch_bounds__(64) void vtm_rules_count_kernel(const RulesArgs a)
{
	__shared__ Shared sh;
	run_utterance<false>(a, blockIdx.x, threadIdx.x, sh);
}

__global__ __launch_bounds__(kScanThreads) void vtm_rules_scan_kernel(const RulesArgs a)
{
	lengths_to_offsets(a.event_offsets_out, a.batch, a.out_capacity, a.status, kRulesNoRoom);
}

__global__ __launch_bounds__(64) void vtm_rules_write_kernel(const RulesArgs a)
{
	__shared__ Shared sh;
	run_utterance<true>(a, blockIdx.x, threadIdx.x, sh);
}

} // namespace

hipError_t launch_generate_events(const RulesArgs& args, hipStream_t stream)
{
	if (args.batch == 0) return hipSuccess;
	const dim3 per_utterance(static_cast<unsigned>(args.batch));
	hipLaunchKernelGGL(vtm_rules_count_kernel, per_utterance, dim3(64), 0, stream, args);
	hipLaunchKernelGGL(vtm_rules_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, args);
	hipLaunchKernelGGL(vtm_rules_write_kernel, per_utterance, dim3(64), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
