// Intonation contours applied to event lists on the device (vtm_intonation.hpp; EventList.cpp:822-900, 1093-1099).
//
// Memory-bound: per utterance 296 x (E read + M written) + 24 x P bytes, against a few dozen double operations per point.
// Three kernels, no scratch:
//   count  one wavefront per utterance, one lane per point: the point's place q_j, the refusals, and by a binary search of
//          the base list's times (read at the events' 296-byte stride) how many base events lie in front of q_j and whether
//          one lies at it.  M = E + the q_j no base event has goes to event_offsets_out[b + 1].
//   scan   one workgroup over the batch: the lengths in place to offsets.  A list that would end beyond out_capacity is
//          dropped there (length 0, status 5), so the sums behind it do not count it: 1024 lengths at a time are summed in
//          parallel, and only a block in which a list does not fit is walked one by one.
//   write  one wavefront per utterance.  It repeats the count's analysis (the same few cache lines; nothing is kept between
//          the kernels), lane j computes the polynomial of point j, and then the merged list leaves as 8-byte units, 37 per
//          event (an event is 296 bytes and 8-byte aligned), 64 consecutive units per store instruction.  A unit finds its
//          source through the points' output places, which are sorted: one search of at most 64 entries in LDS.  Units 0-4
//          of every event (time / has_interp, interp[4]) are rewritten, a new event's other units are +infinity, a base
//          event's are copied as they are (as integers: every bit of a NaN stays).
// Bit parity with the reference: the same double operations in the same order, no FMA contraction (the pragma below and
// the Makefile's flag), IEEE division.
#include "vtm_intonation.hpp"
#include "vtm_offsets_scan.hpp"

namespace gvtm {

namespace {

constexpr int kMaxPoints = GVTM_MAX_INTONATION_POINTS;
static_assert(kMaxPoints == 64, "one lane of the wavefront per point");
static_assert(sizeof(gvtm_event) == 296 && sizeof(gvtm_event) % 8 == 0 && offsetof(gvtm_event, interp) == 8 && offsetof(gvtm_event, param) == 40,
		"an event is 37 units of 8 bytes: time / has_interp, interp[4], param[16], special[16]");
constexpr int kUnits = sizeof(gvtm_event) / 8;
constexpr unsigned long long kInfinityBits = 0x7ff0000000000000ull; // Event::EMPTY_PARAMETER

// What one utterance's wavefront knows after the analysis; lane j holds point j's part (j < n_points)
struct Analysis {
	int32_t status;
	const gvtm_event* base; // the base list
	int64_t n_base;
	int n_points;
	int64_t merged;         // events of the merged list (0 if refused)
	bool smooth;
	// of my point:
	int q;                  // its event's time
	int64_t place;          // its event's index in the merged list
	bool is_new;            // no base event lies at q
	int new_before;         // new events in front of it
	int n_new;
};

__device__ __forceinline__ unsigned long long lanes_below(int lane)
{
	return lane ? ~0ull >> (64 - lane) : 0ull;
}

// One wavefront, all 64 lanes active.  Reads: the utterance's table entries, its points, the last base event's time and
// (search) up to log2(E) + 1 base times per point.
__device__ __forceinline__ Analysis analyse(const IntonationArgs& a, size_t utt, int lane)
{
	Analysis r{};
	r.status = kIntonationOk;
	const int64_t list = a.list_ids ? static_cast<int64_t>(a.list_ids[utt]) : static_cast<int64_t>(utt);
	const int32_t voice = a.voice_ids[utt];
	if (list < 0 || list >= a.n_lists || voice < 0 || voice >= a.n_voices) {
		r.status = kIntonationNoList;
		return r;
	}
	const int64_t first = a.list_offsets[list];
	r.n_base = a.list_offsets[list + 1] - first;
	if (r.n_base <= 0) {
		r.status = kIntonationNoList;
		return r;
	}
	r.base = a.events + first;
	const int64_t first_point = a.point_offsets[utt], n_points = a.point_offsets[utt + 1] - first_point;
	if (n_points < 0 || n_points > kMaxPoints) {
		r.status = kIntonationTooMany;
		return r;
	}
	r.n_points = static_cast<int>(n_points);
	r.smooth = a.voice_k[voice].smooth_intonation != 0;
	const int last_time = r.base[r.n_base - 1].time_ms;
	const bool mine = lane < r.n_points;
	bool bad_time = false;
	if (mine) bad_time = !intonation_point_time(a.points[first_point + lane].time_ms, a.control_period, last_time, r.q);
	if (__ballot(bad_time)) {
		r.status = kIntonationBadTime;
		return r;
	}
	const int q_before = __shfl_up(r.q, 1);
	if (__ballot(mine && lane > 0 && r.q <= q_before)) {
		r.status = kIntonationNotIncreasing;
		return r;
	}
	// base events in front of q: the first index whose time is not below it
	int64_t lo = 0, hi = mine ? r.n_base : 0;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (r.base[mid].time_ms < r.q) lo = mid + 1;
		else hi = mid;
	}
	r.is_new = mine && (lo == r.n_base || r.base[lo].time_ms != r.q);
	const unsigned long long new_lanes = __ballot(r.is_new);
	r.new_before = __popcll(new_lanes & lanes_below(lane));
	r.n_new = __popcll(new_lanes);
	r.place = lo + r.new_before;
	r.merged = r.n_base + r.n_new;
	return r;
}

__global__ __launch_bounds__(64) void vtm_intonation_count_kernel(const IntonationArgs a)
{
	const size_t utt = blockIdx.x;
	const int lane = threadIdx.x;
	const Analysis r = analyse(a, utt, lane);
	if (lane == 0) {
		a.event_offsets_out[utt + 1] = r.merged;
		if (a.status) a.status[utt] = r.status;
	}
}

// event_offsets_out[1 ..= batch] hold the lengths; they leave as the ends of the lists laid back to back, a list that
// would end beyond out_capacity counted as empty (vtm_offsets_scan.hpp)
__global__ __launch_bounds__(kScanThreads) void vtm_intonation_scan_kernel(const IntonationArgs a)
{
	lengths_to_offsets(a.event_offsets_out, a.batch, a.out_capacity, a.status, kIntonationNoRoom);
}

__global__ __launch_bounds__(64) void vtm_intonation_write_kernel(const IntonationArgs a)
{
#pragma clang fp contract(off)
	// the points' events in the merged list, in order, and what they carry; places[n_points ..] are never reached
	__shared__ int64_t places[kMaxPoints];
	__shared__ int times[kMaxPoints];
	__shared__ unsigned char fresh[kMaxPoints];    // the point's event is a new one
	__shared__ unsigned char before[kMaxPoints + 1]; // new events in front of point j's; [n_points]: all of them
	__shared__ double interp[kMaxPoints][4];
	const size_t utt = blockIdx.x;
	const int lane = threadIdx.x;
	const Analysis r = analyse(a, utt, lane);
	if (r.status != kIntonationOk) return;
	// what the scan left: the list's room, or none (status 5); never beyond the output
	const int64_t out_first = a.event_offsets_out[utt], out_end = a.event_offsets_out[utt + 1];
	if (out_first < 0 || out_end > a.out_capacity || out_end - out_first != r.merged) return;

	const bool mine = lane < r.n_points;
	if (mine) {
		const gvtm_intonation_point* pt = a.points + a.point_offsets[utt];
		places[lane] = r.place;
		times[lane] = r.q;
		fresh[lane] = r.is_new;
		before[lane] = static_cast<unsigned char>(r.new_before);
		double c[4] = {0.0, 0.0, 0.0, 0.0};
		if (r.n_points >= 2) {
			const gvtm_intonation_point p1 = pt[lane];
			if (lane + 1 < r.n_points) {
				const gvtm_intonation_point p2 = pt[lane + 1];
				int q2;
				// (its time passed the analysis of lane + 1; evaluated again here rather than carried across lanes)
				(void) intonation_point_time(p2.time_ms, a.control_period, r.base[r.n_base - 1].time_ms, q2);
				intonation_segment(r.smooth, r.q, p1.semitone, p1.slope, q2, p2.semitone, p2.slope, c);
			} else {
				intonation_last(r.smooth, p1.semitone, c);
			}
		}
		interp[lane][0] = c[0];
		interp[lane][1] = c[1];
		interp[lane][2] = c[2];
		interp[lane][3] = c[3];
	}
	if (lane == 0) before[r.n_points] = static_cast<unsigned char>(r.n_new);
	__syncthreads();

	const unsigned long long* src = reinterpret_cast<const unsigned long long*>(r.base);
	unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.events_out + out_first);
	const int64_t n_units = r.merged * kUnits;
	const bool carries = r.n_points >= 2; // rule 6: a single point inserts its event and nothing else
	for (int64_t u = lane; u < n_units; u += 64) {
		const int64_t m = u / kUnits;
		const int c = static_cast<int>(u - m * kUnits);
		// first point whose event is not in front of event m
		int lo = 0, hi = r.n_points;
		while (lo < hi) {
			const int mid = (lo + hi) >> 1;
			if (places[mid] < m) lo = mid + 1;
			else hi = mid;
		}
		const bool at_point = lo < r.n_points && places[lo] == m;
		const bool is_new = at_point && fresh[lo];
		const int64_t source = (m - before[lo]) * kUnits + c; // (not read for a new event)
		unsigned long long v;
		if (c == 0) {
			const unsigned time = is_new ? static_cast<unsigned>(times[lo]) : static_cast<unsigned>(src[source]); // little endian: time_ms is the low half
			v = static_cast<unsigned long long>(time) | (at_point && carries ? 1ull << 32 : 0ull);
		} else if (c < 5) {
			v = at_point && carries ? static_cast<unsigned long long>(__double_as_longlong(interp[lo][c - 1])) : 0ull;
		} else {
			v = is_new ? kInfinityBits : src[source];
		}
		dst[u] = v;
	}
}

} // namespace

hipError_t launch_apply_intonation(const IntonationArgs& args, hipStream_t stream)
{
	if (args.batch == 0) return hipSuccess;
	const dim3 per_utterance(static_cast<unsigned>(args.batch));
	hipLaunchKernelGGL(vtm_intonation_count_kernel, per_utterance, dim3(64), 0, stream, args);
	hipLaunchKernelGGL(vtm_intonation_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, args);
	hipLaunchKernelGGL(vtm_intonation_write_kernel, per_utterance, dim3(64), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
