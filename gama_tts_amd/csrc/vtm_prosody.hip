// Rhythm and intonation points on the device (vtm_prosody.hpp; EventList.cpp:687-793, 796-819, 903-927).
//
// Rhythm: one kernel, one lane per foot of the batch.  A lane finds its utterance in the foot offsets (a binary search),
// checks its foot against the utterance's postures and the foot in front of it, and multiplies the tempi of its postures;
// feet are disjoint, so no lane reads what another writes.  The largest status of an utterance's feet is the utterance's.
//
// Points: three kernels, no scratch, one wavefront per utterance in the first and the last:
//   count  lanes take posture ids, feet and groups for the structure checks; then lane L takes the L-th foot that lies in a
//          group (at most 63 of them once the count has passed) for what stands alone per foot -- the vocoid search, the rule
//          lookups and the raw semitone, slope and offset -- and stages one or two raw points in LDS at the rank a ballot of
//          the marked feet gives it; lane 0 then walks the minTime chain over the staged points (prosody_chain, the host's
//          text).  Leaves the number of points and the status.
//   scan   lengths to offsets (vtm_offsets_scan.hpp); points that do not fit are dropped with status 5.
//   write  the same again (nothing is kept between the kernels but the offsets); the points leave as 8-byte units, three per
//          point, consecutive lanes to consecutive units.
// Bit parity with the host: every value comes from the inline functions of vtm_prosody.hpp; no FMA contraction.
#include "vtm_prosody.hpp"
#include "vtm_offsets_scan.hpp"

namespace gvtm {

namespace {

static_assert(kProsodyMaxPoints == 64, "the points of an utterance are staged by one wavefront");
static_assert(sizeof(gvtm_intonation_point) == 24, "a point is three units of 8 bytes");
static_assert(sizeof(gvtm_foot) == 24 && sizeof(gvtm_tone_group) == 32 && sizeof(gvtm_posture) == 24 && sizeof(gvtm_rule_data) == 48, "the tables' records");

constexpr int kRhythmThreads = 256;

__device__ __forceinline__ unsigned long long lanes_below(int lane)
{
	return lane ? ~0ull >> (64 - lane) : 0ull;
}

__global__ __launch_bounds__(kRhythmThreads) void vtm_prosody_rhythm_kernel(const ProsodyRhythmArgs a)
{
#pragma clang fp contract(off)
	const int64_t f = static_cast<int64_t>(blockIdx.x) * kRhythmThreads + threadIdx.x;
	if (f >= a.n_feet) return;
	// the utterance that owns foot f: the last one whose feet start at or in front of it
	size_t lo = 0, hi = a.batch;
	while (lo < hi) {
		const size_t mid = lo + (hi - lo + 1) / 2;
		if (mid < a.batch && a.foot_offsets[mid] <= f) lo = mid;
		else hi = mid - 1;
	}
	const size_t utt = lo;
	const int64_t first_foot = a.foot_offsets[utt], end_foot = a.foot_offsets[utt + 1];
	if (first_foot < 0 || f < first_foot || f >= end_foot || end_foot > a.n_feet) return; // (offsets that are no table: no utterance owns the foot)
	const int64_t first_posture = a.posture_offsets[utt], end_posture = a.posture_offsets[utt + 1];
	int32_t status = kProsodyOk;
	if (first_posture < 0 || end_posture < first_posture || end_posture > a.n_postures ||
			!prosody_foot_ok(a.feet + first_foot, f - first_foot, end_posture - first_posture)) {
		status = kProsodyBadStructure;
	} else {
		const gvtm_foot foot = a.feet[f];
		const double tempo = prosody_foot_tempo(a.config, foot);
		if (!prosody_finite(tempo)) {
			status = kProsodyBadValue;
		} else {
			gvtm_posture* p = a.postures_out + first_posture;
			for (int j = foot.start; j < foot.end + 1; j++) p[j].tempo *= tempo;
		}
	}
	if (status != kProsodyOk && a.status) atomicMax(&a.status[utt], status);
}

// the LDS of one utterance's wavefront
struct Shared {
	ProsodyRawPoint raw[kProsodyMaxPoints];
	gvtm_intonation_point points[kProsodyMaxPoints];
	int finite;
};

// One utterance, one wavefront, all 64 lanes active: the status, and in sh.points the `count` points it returns
__device__ __forceinline__ int place_utterance(const ProsodyPlaceArgs& a, size_t utt, int lane, Shared& sh, int32_t& status)
{
#pragma clang fp contract(off)
	status = kProsodyOk;
	const int64_t first_posture = a.posture_offsets[utt], n_postures = a.posture_offsets[utt + 1] - first_posture;
	const int64_t first_foot = a.foot_offsets[utt], n_feet = a.foot_offsets[utt + 1] - first_foot;
	const int64_t first_group = a.group_offsets[utt], n_groups = a.group_offsets[utt + 1] - first_group;
	const int32_t rule_status = a.status ? a.status[utt] : 0;
	if (first_posture < 0 || first_foot < 0 || first_group < 0 || n_postures < 0 || n_feet < 0 || n_groups < 0 || n_postures > 0x7fffffff ||
			n_feet > 0x7fffffff || n_groups > 0x7fffffff) {
		status = kProsodyBadStructure;
		return 0;
	}
	const gvtm_posture* postures = a.postures + first_posture;
	const gvtm_foot* feet = a.feet + first_foot;
	const gvtm_tone_group* groups = a.groups + first_group;
	bool bad = false;
	for (int64_t i = lane; i < n_postures; i += 64) bad = bad || postures[i].posture < 0 || postures[i].posture >= a.n_vocoid;
	for (int64_t i = lane; i < n_feet; i += 64) bad = bad || !prosody_foot_ok(feet, i, n_postures);
	for (int64_t g = lane; g < n_groups; g += 64) bad = bad || !prosody_group_ok(groups, g, n_feet);
	if (__ballot(bad)) {
		status = kProsodyBadStructure;
		return 0;
	}
	if (a.rhythm_status && a.rhythm_status[utt] != kProsodyOk) {
		status = a.rhythm_status[utt];
		return 0;
	}
	const int64_t n_rows = a.rule_counts[utt];
	if (rule_status != 0 || n_rows <= 0 || n_rows > a.max_rules || n_rows > 0x7fffffff) {
		status = kProsodyNoRules;
		return 0;
	}
	if (a.voice_k && a.voice_ids) {
		const int32_t voice = a.voice_ids[utt];
		if (voice < 0 || voice >= a.n_voices || a.voice_k[voice].macro_intonation == 0) return 0; // (a voice outside the plan's: the apply entry refuses it)
	}
	if (n_groups == 0) return 0;
	// feet in groups: the groups' lengths (they are disjoint and inside the feet, so the sum is at most n_feet)
	int64_t in_groups = 0;
	for (int64_t g = lane; g < n_groups; g += 64) in_groups += groups[g].end_foot - groups[g].start_foot + 1;
	for (int step = 32; step > 0; step >>= 1) in_groups += __shfl_xor(in_groups, step);
	if (in_groups + 1 > kProsodyMaxPoints) {
		status = kProsodyTooMany;
		return 0;
	}
	// lane L < in_groups: the L-th of those feet.  (Every group holds a foot, so there are at most 63 groups.)
	const int n_in = static_cast<int>(in_groups);
	const bool mine = lane < n_in;
	int g_mine = 0, j_mine = 0;
	if (mine) {
		int rest = lane;
		for (int g = 0; g < static_cast<int>(n_groups); ++g) {
			const int length = groups[g].end_foot - groups[g].start_foot + 1;
			if (rest < length) {
				g_mine = g;
				j_mine = groups[g].start_foot + rest;
				break;
			}
			rest -= length;
		}
	}
	const bool marked = mine && feet[j_mine].marked != 0;
	const unsigned long long marked_lanes = __ballot(marked);
	const int count = n_in + __popcll(marked_lanes) + 1;
	if (count > kProsodyMaxPoints) {
		status = kProsodyTooMany;
		return 0;
	}
	const gvtm_rule_data* rows = a.rule_data + utt * static_cast<size_t>(a.max_rules);
	const double* onsets = a.onsets + first_posture;
	const int n_rules = static_cast<int>(n_rows);
	bool no_rule = false, finite = true;
	if (mine) {
		const gvtm_tone_group t = groups[g_mine];
		const gvtm_foot foot = feet[j_mine];
		const double start_time = onsets[feet[t.start_foot].start];
		const double end_time = onsets[feet[t.end_foot].end];
		const double pretonic_delta = prosody_pretonic_delta(t.param, start_time, end_time);
		for (int k = 0; k < 5; ++k) finite = finite && prosody_finite(t.param[k]);
		const double* d = a.draws ? a.draws + 2 * (first_foot + j_mine) : nullptr;
		if (d) finite = finite && prosody_finite(d[0]) && prosody_finite(d[1]);
		const int posture = prosody_vocoid_posture(a.vocoid, postures, foot);
		const int rule = prosody_rule_of(rows, n_rules, 0, posture);
		const int at = lane + __popcll(marked_lanes & lanes_below(lane));
		if (rule < 0) {
			no_rule = true;
		} else {
			ProsodyRawPoint p;
			p.beat = rows[rule].beat;
			p.offset = lane == 0 ? 0.0 : static_cast<double>(a.config.time_offset);
			if (!foot.marked) {
				prosody_pretonic(a.config, t.param, d, onsets[posture], start_time, pretonic_delta, p.semitone, p.slope);
				sh.raw[at] = p;
			} else {
				prosody_tonic(a.config, t.param, t.type, d, p.semitone, p.slope);
				sh.raw[at] = p;
				const int rule2 = prosody_rule_of(rows, n_rules, rule, foot.end);
				if (rule2 < 0) no_rule = true;
				else sh.raw[at + 1] = ProsodyRawPoint{rows[rule2].beat, 0.0, prosody_boundary(t.param), 0.0};
			}
		}
	} else if (lane == n_in) {
		sh.raw[count - 1] = ProsodyRawPoint{rows[n_rules - 1].beat, 0.0, prosody_boundary(groups[n_groups - 1].param), 0.0};
	}
	if (__ballot(no_rule)) {
		status = kProsodyNoRules;
		return 0;
	}
	const bool all_finite = __ballot(!finite) == 0;
	__syncthreads();
	if (lane == 0) sh.finite = prosody_chain(a.config, a.control_period, sh.raw, count, sh.points) ? 1 : 0;
	__syncthreads();
	if (!all_finite || !sh.finite) {
		status = kProsodyBadValue;
		return 0;
	}
	return count;
}

__global__ __launch_bounds__(64) void vtm_prosody_count_kernel(const ProsodyPlaceArgs a)
{
	__shared__ Shared sh;
	const size_t utt = blockIdx.x;
	int32_t status;
	const int count = place_utterance(a, utt, threadIdx.x, sh, status);
	__syncthreads(); // (every lane has read the rules entry's status)
	if (threadIdx.x == 0) {
		a.point_offsets_out[utt + 1] = count;
		if (a.status) a.status[utt] = status;
	}
}

__global__ __launch_bounds__(kScanThreads) void vtm_prosody_scan_kernel(const ProsodyPlaceArgs a)
{
	lengths_to_offsets(a.point_offsets_out, a.batch, a.points_capacity, a.status, kProsodyNoRoom);
}

__global__ __launch_bounds__(64) void vtm_prosody_write_kernel(const ProsodyPlaceArgs a)
{
	__shared__ Shared sh;
	const size_t utt = blockIdx.x;
	const int lane = threadIdx.x;
	// (the status is now the count's or the scan's: an utterance it refuses is refused again below, whatever for)
	int32_t status;
	const int count = place_utterance(a, utt, lane, sh, status);
	if (a.list_ids_out && lane == 0) a.list_ids_out[utt] = (a.status ? a.status[utt] : status) == kProsodyOk ? static_cast<int32_t>(utt) : -1;
	if (status != kProsodyOk || count == 0) return;
	const int64_t out_first = a.point_offsets_out[utt], out_end = a.point_offsets_out[utt + 1];
	if (out_first < 0 || out_end > a.points_capacity || out_end - out_first != count) return;
	const unsigned long long* src = reinterpret_cast<const unsigned long long*>(sh.points);
	unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.points_out + out_first);
	for (int u = lane; u < 3 * count; u += 64) dst[u] = src[u];
}

} // namespace

hipError_t launch_apply_rhythm(const ProsodyRhythmArgs& args, hipStream_t stream)
{
	if (args.batch == 0 || args.n_feet <= 0) return hipSuccess;
	const int64_t blocks = (args.n_feet + kRhythmThreads - 1) / kRhythmThreads;
	hipLaunchKernelGGL(vtm_prosody_rhythm_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kRhythmThreads), 0, stream, args);
	return hipGetLastError();
}

hipError_t launch_place_intonation(const ProsodyPlaceArgs& args, hipStream_t stream)
{
	if (args.batch == 0) return hipSuccess;
	const dim3 per_utterance(static_cast<unsigned>(args.batch));
	hipLaunchKernelGGL(vtm_prosody_count_kernel, per_utterance, dim3(64), 0, stream, args);
	hipLaunchKernelGGL(vtm_prosody_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, args);
	hipLaunchKernelGGL(vtm_prosody_write_kernel, per_utterance, dim3(64), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
