// Device helpers shared by the synthesis kernels (included inside namespace gvtm { namespace { ).
#pragma once

// ----------------------------------------------------------------------------------
// cross-lane helpers (one tube section per lane; a DPP row is 16 lanes)

constexpr int kDppRowShr1 = 0x111; // lane i <- lane i-1 within the row, 0 shifted in
constexpr int kDppRowShl1 = 0x101; // lane i <- lane i+1 within the row, 0 shifted in

__device__ __forceinline__ float from_left(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kDppRowShr1, 0xF, 0xF, true));
}
__device__ __forceinline__ float from_right(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kDppRowShl1, 0xF, 0xF, true));
}
__device__ __forceinline__ double from_left(double v)
{
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kDppRowShr1, 0xF, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kDppRowShr1, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_right(double v)
{
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kDppRowShl1, 0xF, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kDppRowShl1, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}
template <int LANE>
__device__ __forceinline__ float lane_value(float v)
{
	return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), LANE));
}
template <int LANE>
__device__ __forceinline__ double lane_value(double v)
{
	const int lo = __builtin_amdgcn_readlane(__double2loint(v), LANE);
	const int hi = __builtin_amdgcn_readlane(__double2hiint(v), LANE);
	return __hiloint2double(hi, lo);
}

// Row broadcast (DPP row_newbcast:N, gfx90a+): every lane of a 16-lane row receives lane N of ITS row.
// A 64-bit value moves in one v_mov_b64_dpp (row_newbcast is the one DPP control the fp64 pipe accepts);
// the clang builtin only covers 32-bit operands, so the intrinsic is named directly.
extern "C" __device__ double gvtm_update_dpp_f64(double, double, int, int, int, bool) __asm("llvm.amdgcn.update.dpp.f64");
template <int N>
__device__ __forceinline__ float row_bcast(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + N, 0xF, 0xF, true));
}
template <int N>
__device__ __forceinline__ double row_bcast(double v)
{
	return gvtm_update_dpp_f64(0.0, v, 0x150 + N, 0xF, 0xF, true);
}

// DPP row rotate: lane i of a row receives lane (i - N) mod 16 (every cross-lane primitive here is checked on the device by
// tests/test_gpu_parity.py through the diagnostics library's dpp_selftest_kernel, vtm_diag_kernels.hip).
template <int N>
__device__ __forceinline__ double row_rotate(double v)
{
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x120 + N, 0xF, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x120 + N, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}

template <int N>
__device__ __forceinline__ float row_rotate(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xF, 0xF, true));
}

// Wave-wide DPP shifts (gfx9 wave_shr:1 / wave_shl:1): lane i receives lane i-1 / i+1 of the whole
// wavefront, 0 is shifted in at the ends.
__device__ __forceinline__ double from_left_wave(double v)
{
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xF, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_right_wave(double v)
{
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xF, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float from_left_wave(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float from_right_wave(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xF, 0xF, true));
}


// A product that the reference rounds before it is added to something.  With TFloat = float the
// device path reproduces that rounding (bit parity with VocalTractModel0<float>: the float model's
// oscillator phase and filter states leave no slack); in fp64 the product may fuse into the
// following add (differences ~1e-16, far inside the 1e-9 parity bar).
__device__ __forceinline__ double rmul(double a, double b)
{
	return a * b;
}
__device__ __forceinline__ float rmul(float a, float b)
{
#pragma clang fp contract(off)
	return a * b;
}

// Util::amplitude60dB (vtm/VTMUtil.h:48-67)
template <bool FAR_INLINE = false>
__device__ __forceinline__ double amplitude_60db_dev(double db)
{
	if (db <= 0.0) return 0.0;
	if (db == 60.0) return 1.0;
	return vmath::exp10_short((db - 60.0) * (1.0 / 20.0));
}
// TFloat = float: std::pow(10.0f, x) is powf, reproduced bit for bit (vtm_math.hpp)
// (FAR_INLINE, here and below: the float routine's library fallback in line instead of as a cold call; nothing in double)
template <bool FAR_INLINE = false>
__device__ __forceinline__ float amplitude_60db_dev(float db)
{
	if (db <= 0.0f) return 0.0f;
	if (db == 60.0f) return 1.0f;
	const float y = rmul(db - 60.0f, static_cast<float>(1.0 / 20.0));
	return vmath::powf_base10<FAR_INLINE>(y);
}

// Util::frequency (vtm/VTMUtil.h:74-84)
template <bool FAR_INLINE = false>
__device__ __forceinline__ double frequency_dev(double pitch)
{
	return 220.0 * vmath::exp2_short((pitch + 3.0) * (1.0 / 12.0));
}
template <bool FAR_INLINE = false>
__device__ __forceinline__ float frequency_dev(float pitch)
{
	const float x = rmul(pitch + 3.0f, static_cast<float>(1.0 / 12.0));
	return rmul(220.0f, vmath::powf_base2<FAR_INLINE>(x));
}

// std::tan / std::cos of BandpassFilter::update (BandpassFilter.h:105-106): tanf / cosf for TFloat = float
template <bool FAR_INLINE = false> __device__ __forceinline__ double tan_dev(double t) { return vmath::tan_short(t); }
template <bool FAR_INLINE = false> __device__ __forceinline__ double cos_dev(double t) { return vmath::cos_short(t); }
template <bool FAR_INLINE = false> __device__ __forceinline__ float tan_dev(float t) { return vmath::tanf_glibc<FAR_INLINE>(t); }
template <bool FAR_INLINE = false> __device__ __forceinline__ float cos_dev(float t) { return vmath::cosf_glibc<FAR_INLINE>(t); }

template <typename T> struct Pair;
template <> struct Pair<double> { using type = double2; };
template <> struct Pair<float> { using type = float2; };

// NoiseSource::getSample (vtm/NoiseSource.h:40-44): seed = frac(seed * 377).  The sequence is
// chaotic, so the product has to be rounded to double before the integer part is removed,
// exactly as the reference does — a contracted fma(seed, 377, -floor(p)) decorrelates the
// sequence within a few steps (SURVEY.md hard part 5).
__device__ __forceinline__ double noise_advance(double seed)
{
#pragma clang fp contract(off)
	const double product = seed * 377.0;
	return product - floor(product);
}

// a / b in float for operands whose quotient, numerator and denominator are far from the ends of the exponent range
// (squared radii between 1e-4 and some hundreds, their sums and differences): the division's own refinement steps
// (reciprocal, two Newton steps, quotient, two residual corrections -- what the compiler emits for a / b) without its
// range scaling and its fix-up of infinities, NaNs and denormals, i.e. 8 instead of 11 instructions with the same
// correctly rounded result (pinned against IEEE division over the whole operand range in tests/test_gpu_parity_f32.py).
__device__ __forceinline__ float fdiv_n(float a, float b)
{
	float r = __builtin_amdgcn_rcpf(b);
	const float e0 = __builtin_fmaf(-b, r, 1.0f);
	r = __builtin_fmaf(e0, r, r);
	float q = a * r;
	const float e1 = __builtin_fmaf(-b, q, a);
	q = __builtin_fmaf(e1, r, q);
	const float e2 = __builtin_fmaf(-b, q, a);
	return __builtin_fmaf(e2, r, q);
}
__device__ __forceinline__ double fdiv_n(double a, double b) { return a / b; }

// One step of Controller::synthesize's float32 running sum (Controller.cpp:308-310); kept
// out of FMA contraction so that the per-step parameter values are bit-exact.
__device__ __forceinline__ float interp_delta(float next, float cur, float coef)
{
#pragma clang fp contract(off)
	const float diff = next - cur;
	return diff * coef;
}
__device__ __forceinline__ float interp_advance(float cur, float delta)
{
#pragma clang fp contract(off)
	return cur + delta;
}

template <typename TT>
struct SrcTap {
	TT h, dh;
};


// Glottal wavetable entry i for the current source amplitude.  With tn_delta == 0 (every
// shipped voice) the table is static; otherwise WavetableGlottalSource::setup
// (vtm/WavetableGlottalSource.h:162-184) rewrites the falling part as a pure function of
// the amplitude, which is evaluated here on demand.
__device__ __forceinline__ double wavetable_entry(const double* table, const DeviceConstants& k, unsigned i, double ax)
{
	if (k.tn_delta == 0.0 || k.waveform != 0 || i < k.table_div1 || i >= k.table_div2) return table[i];
	double new_div2 = static_cast<double>(k.table_div2) - rint(ax * k.tn_delta);
	new_div2 = new_div2 > 0.0 ? new_div2 : 0.0;
	if (i >= static_cast<unsigned>(new_div2)) return 0.0;
	const double inv = 1.0 / (new_div2 - static_cast<double>(k.table_div1));
	const double x = static_cast<double>(i - k.table_div1) * inv;
	return 1.0 - (x * x);
}
// TFloat = float: the reference steps x by repeated addition (x += invNewTnLength, :178); in float
// that differs from the product by several ulp, so the additions are replayed (only voices with
// tn_min != tn_max take this path)
__device__ __forceinline__ float wavetable_entry(const float* table, const DeviceConstants& k, unsigned i, float ax)
{
	if (k.tn_delta == 0.0 || k.waveform != 0 || i < k.table_div1 || i >= k.table_div2) return table[i];
	float new_div2 = static_cast<float>(k.table_div2) - rintf(ax * static_cast<float>(k.tn_delta));
	new_div2 = new_div2 > 0.0f ? new_div2 : 0.0f;
	if (i >= static_cast<unsigned>(new_div2)) return 0.0f;
	const float inv = 1.0f / (new_div2 - static_cast<float>(k.table_div1));
	float x = 0.0f;
	for (unsigned j = k.table_div1; j < i; ++j) x += inv;
	return 1.0f - rmul(x, x);
}
