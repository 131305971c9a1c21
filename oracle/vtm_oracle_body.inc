/* ------------------------------------------------------------------------- */
/* vtm/VTMUtil.h                                                              */

/* Util::amplitude60dB, vtm/VTMUtil.h:48-67 */
static real amplitude60dB(real db)
{
	if (db <= RC(0.0)) return RC(0.0);
	if (db == RC(60.0)) return RC(1.0);
	db -= RC(60.0);
	return R_POW(RC(10.0), db * RC(1.0 / 20.0));
}

/* Util::frequency, vtm/VTMUtil.h:74-84 */
static real frequency(real pitch)
{
	return RC(220.0) * R_POW(RC(2.0), (pitch + RC(3.0)) * RC(1.0 / 12.0));
}

/* ------------------------------------------------------------------------- */
/* vtm/WavetableGlottalSourceFIRFilter.h                                      */

#define FIR_LIMIT 200

/* rationalApproximation, WavetableGlottalSourceFIRFilter.h:316-361 */
static void rational_approximation(real number, int* order, int* numerator, int* denominator)
{
	if (*order <= 0) {
		*numerator = 0;
		*denominator = 0;
		*order = -1;
		return;
	}
	const real fractional = R_FABS(number - (int) number);
	int order_max = 2 * (*order);
	if (order_max > FIR_LIMIT) order_max = FIR_LIMIT;

	real min_error = RC(1.0);
	int modulus = 0;
	for (int i = *order; i <= order_max; ++i) {
		const real ps = i * fractional;
		const int ip = (int) (ps + RC(0.5));
		const real error = (real) fabs((ps - (double) ip) / i); /* the reference casts ip to double here (:339) */
		if (error < min_error) {
			min_error = error;
			modulus = ip;
			*denominator = i;
		}
	}
	*numerator = (int) R_FABS(number) * (*denominator) + modulus;
	if (number < RC(0.0)) *numerator *= -1;
	*order = *denominator - 1;
	if (*numerator == *denominator) {
		*denominator = order_max;
		*order = *numerator = *denominator - 1;
	}
}

/* maximallyFlat, WavetableGlottalSourceFIRFilter.h:137-215 (beta/gamma range
 * checks omitted: the caller passes the fixed 0.2 / 0.1 of WavetableGlottalSource.h:94-95) */
static void maximally_flat(real beta, real gamma, int* np, real* coefficient)
{
	real a[FIR_LIMIT + 1], c[FIR_LIMIT + 1];
	int numerator;

	memset(a, 0, sizeof(a));
	memset(c, 0, sizeof(c));
	*np = 0;
	int nt = (int) (RC(1.0) / (RC(4.0) * gamma * gamma));
	const real ac = (RC(1.0) + R_COS((RC(2.0) * RC(M_PI)) * beta)) / RC(2.0);
	rational_approximation(ac, &nt, &numerator, np);

	const int n = (2 * (*np)) - 1;
	if (numerator == 0) numerator = 1;

	c[1] = a[1] = RC(1.0);
	const int ll = nt - numerator;
	for (int i = 2; i <= *np; ++i) {
		c[i] = R_COS((RC(2.0) * RC(M_PI)) * ((real) (i - 1) / n));
		const real x = (RC(1.0) - c[i]) / RC(2.0);
		real y = x;
		if (numerator == nt) continue;
		real sum = RC(1.0);
		for (int j = 1; j <= ll; ++j) {
			real z = y;
			if (numerator != 1) {
				for (int jj = 1; jj <= (numerator - 1); ++jj) {
					z *= RC(1.0) + ((real) j / jj);
				}
			}
			y *= x;
			sum += z;
		}
		a[i] = (real) (sum * pow((double) (RC(1.0) - x), (double) numerator)); /* std::pow(TFloat, int) is evaluated in double */
	}
	for (int i = 1; i <= *np; ++i) {
		coefficient[i] = a[1] / RC(2.0);
		for (int j = 2; j <= *np; ++j) {
			int m = ((i - 1) * (j - 1)) % n;
			if (m > nt) m = n - m;
			coefficient[i] += c[m + 1] * a[j];
		}
		coefficient[i] *= RC(2.0) / (real) n;
	}
}

/* ctor, WavetableGlottalSourceFIRFilter.h:74-114 with trim (:227-235);
 * beta 0.2, gamma 0.1, cutoff 1e-8 from WavetableGlottalSource.h:94-96 */
int PUB(vtmo_fir_coefficients)(real* coef)
{
	int nc;
	real coefficient[FIR_LIMIT + 1];
	maximally_flat(RC(0.2), RC(0.1), &nc, coefficient);
	for (int i = nc; i > 0; --i) {
		if (R_FABS(coefficient[i]) >= R_FABS(RC(0.00000001))) {
			nc = i;
			break;
		}
	}
	const int taps = (nc * 2) - 1;
	int increment = -1;
	int pointer = nc;
	for (int i = 0; i < taps; ++i) {
		coef[i] = coefficient[pointer];
		pointer += increment;
		if (pointer <= 0) {
			pointer = 2;
			increment = 1;
		}
	}
	return taps;
}

/* ------------------------------------------------------------------------- */
/* vtm/WavetableGlottalSource.h                                               */

typedef struct {
	unsigned div1, div2;
	real tn_length, tn_delta, basic_increment, position, prev_amplitude;
	real table[VTMO_WAVETABLE_LENGTH];
	int taps, ptr;
	real coef[VTMO_FIR_MAX_TAPS];
	real data[VTMO_FIR_MAX_TAPS];
	double* tap_pos; /* optional debug tap */
} glottal_source;

/* ctor, WavetableGlottalSource.h:90-141 */
static void glottal_init(glottal_source* g, int waveform, real sample_rate, real tp, real tn_min, real tn_max)
{
	const unsigned len = VTMO_WAVETABLE_LENGTH;
	g->div1 = (unsigned) R_RINT(len * (tp / RC(100.0)));
	g->div2 = (unsigned) R_RINT(len * ((tp + tn_max) / RC(100.0)));
	g->tn_length = g->div2 - g->div1;
	g->tn_delta = R_RINT(len * ((tn_max - tn_min) / RC(100.0)));
	g->basic_increment = len / sample_rate;
	g->position = RC(0.0);
	g->prev_amplitude = -RC(1.0);
	if (waveform == 0) {
		for (unsigned i = 0; i < g->div1; ++i) {
			const real x = (real) i / g->div1;
			const real x2 = x * x;
			const real x3 = x2 * x;
			g->table[i] = (RC(3.0) * x2) - (RC(2.0) * x3);
		}
		for (unsigned i = g->div1, j = 0; i < g->div2; ++i, ++j) {
			const real x = (real) j / g->tn_length;
			g->table[i] = RC(1.0) - (x * x);
		}
		for (unsigned i = g->div2; i < len; ++i) g->table[i] = RC(0.0);
	} else {
		for (unsigned i = 0; i < len; ++i) {
			g->table[i] = R_SIN(((real) i / len) * RC(2.0) * RC(M_PI));
		}
	}
	g->taps = PUB(vtmo_fir_coefficients)(g->coef);
	memset(g->data, 0, sizeof(g->data));
	g->ptr = 0;
}

void PUB(vtmo_wavetable)(const vtmo_config* cfg, int sample_rate, real* table)
{
	glottal_source g;
	glottal_init(&g, cfg->waveform, (real) sample_rate, (real) cfg->glottal_pulse_tp, (real) cfg->glottal_pulse_tn_min, (real) cfg->glottal_pulse_tn_max);
	memcpy(table, g.table, sizeof(g.table));
}

/* setup, WavetableGlottalSource.h:162-184 */
static void glottal_setup(glottal_source* g, real amplitude)
{
	if (g->tn_delta == RC(0.0) || amplitude == g->prev_amplitude) return;
	g->prev_amplitude = amplitude;
	real new_div2 = g->div2 - R_RINT(amplitude * g->tn_delta);
	if (new_div2 < RC(0.0)) new_div2 = RC(0.0);
	const real inv = RC(1.0) / (new_div2 - g->div1);
	real x = RC(0.0);
	for (unsigned i = g->div1, end = (unsigned) new_div2; i < end; ++i, x += inv) {
		g->table[i] = RC(1.0) - (x * x);
	}
	for (unsigned i = (unsigned) new_div2; i < g->div2; ++i) g->table[i] = RC(0.0);
}

/* mod0, WavetableGlottalSource.h:265-272 */
static real mod0(real v)
{
	if (v > (real) (VTMO_WAVETABLE_LENGTH - 1)) v -= (real) VTMO_WAVETABLE_LENGTH;
	return v;
}

/* filter, WavetableGlottalSourceFIRFilter.h:276-304 */
static real fir_filter(glottal_source* g, real input, int need_output)
{
	if (need_output) {
		real output = RC(0.0);
		g->data[g->ptr] = input;
		for (int i = 0; i < g->taps; ++i) {
			output += g->data[g->ptr] * g->coef[i];
			if (++g->ptr >= g->taps) g->ptr = 0;
		}
		if (--g->ptr < 0) g->ptr = g->taps - 1;
		return output;
	}
	g->data[g->ptr] = input;
	if (--g->ptr < 0) g->ptr = g->taps - 1;
	return RC(0.0);
}

/* getSample (2x oversampling oscillator), WavetableGlottalSource.h:212-235.
 * The cast of a position in (-1, 0) to unsigned goes through a signed
 * truncation (what x86-64 g++ emits for double -> unsigned int), i.e. 0. */
static real glottal_sample(glottal_source* g, real freq)
{
	real output = RC(0.0);
	for (int i = 0; i < 2; ++i) {
		g->position = mod0(g->position + ((freq / RC(2.0)) * g->basic_increment));
		if (g->tap_pos) g->tap_pos[i] = g->position;
		const unsigned lower = (unsigned) (long long) g->position;
		const unsigned upper = (unsigned) (long long) mod0((real) (lower + 1));
		const real v = g->table[lower] + ((g->position - lower) * (g->table[upper] - g->table[lower]));
		output = fir_filter(g, v, i);
	}
	return output;
}

/* ------------------------------------------------------------------------- */
/* vtm/SampleRateConverter.h                                                  */

enum {
	SRC_BUFFER_SIZE = 1024,
	SRC_L_BITS = 8,
	SRC_L_RANGE = 256,
	SRC_M_BITS = 8,
	SRC_M_RANGE = 256,
	SRC_ZERO_CROSSINGS = 13,
	SRC_FILTER_LENGTH = VTMO_SRC_FILTER_LENGTH,
	SRC_FRACTION_BITS = 16,
	SRC_FRACTION_RANGE = 65536,
	SRC_FILTER_LIMIT = VTMO_SRC_FILTER_LENGTH - 1
};
#define SRC_M_MASK 0x000000FFu
#define SRC_L_MASK 0x0000FF00u
#define SRC_FRACTION_MASK 0x0000FFFFu
#define SRC_N_MASK 0xFFFF0000u

typedef struct {
	real ratio;
	int fill_ptr, empty_ptr, pad_size, fill_size;
	unsigned time_register_increment, filter_increment, phase_increment, time_register;
	int fill_counter;
	int count_only;
	real h[SRC_FILTER_LENGTH], delta_h[SRC_FILTER_LENGTH], buffer[SRC_BUFFER_SIZE];
	float* out;
	size_t out_cap, out_n;
} src_state;

/* Izero, SampleRateConverter.h:175-194 */
static real izero(real x)
{
	real sum, u, halfx, temp;
	int n;
	sum = u = n = 1;
	halfx = x / RC(2.0);
	do {
		temp = halfx / n;
		n += 1;
		temp *= temp;
		u *= temp;
		sum += u;
	} while (u >= RC(1E-21) * sum);
	return sum;
}

/* initializeFilter, SampleRateConverter.h:230-255 */
void PUB(vtmo_src_filter)(real* h, real* delta_h)
{
	const real beta = RC(5.658);
	const real lp_cutoff = RC(11.0 / 13.0);
	h[0] = lp_cutoff;
	const real x = RC(M_PI / SRC_L_RANGE);
	for (unsigned i = 1; i < SRC_FILTER_LENGTH; ++i) {
		const real y = i * x;
		h[i] = R_SIN(y * lp_cutoff) / y;
	}
	const real ibeta = RC(1.0) / izero(beta);
	for (unsigned i = 0; i < SRC_FILTER_LENGTH; ++i) {
		const real temp = (real) i / SRC_FILTER_LENGTH;
		h[i] *= izero(beta * R_SQRT(RC(1.0) - (temp * temp))) * ibeta;
	}
	for (unsigned i = 0; i < SRC_FILTER_LIMIT; ++i) delta_h[i] = h[i + 1] - h[i];
	delta_h[SRC_FILTER_LIMIT] = RC(0.0) - h[SRC_FILTER_LIMIT];
}

/* initializeConversion + initializeBuffer + reset, SampleRateConverter.h:136-164, :206-218, :119-125 */
static void src_init(src_state* s, real input_rate, real output_rate, int count_only)
{
	memset(s, 0, sizeof(*s));
	s->count_only = count_only;
	if (!count_only) PUB(vtmo_src_filter)(s->h, s->delta_h);
	s->ratio = output_rate / input_rate;
	s->time_register_increment = (unsigned) rint(pow(2.0, SRC_FRACTION_BITS) / s->ratio); /* double arithmetic (:145) */
	const real rounded_ratio = (real) (pow(2.0, SRC_FRACTION_BITS) / s->time_register_increment);
	if (s->ratio >= RC(1.0)) {
		s->filter_increment = SRC_L_RANGE;
	} else {
		s->phase_increment = (unsigned) R_RINT(s->ratio * SRC_FRACTION_RANGE);
	}
	s->pad_size = (s->ratio >= RC(1.0)) ? (int) SRC_ZERO_CROSSINGS : (int) (SRC_ZERO_CROSSINGS / rounded_ratio) + 1;
	s->fill_ptr = s->pad_size;
	s->fill_size = SRC_BUFFER_SIZE - (2 * s->pad_size);
}

static void src_emit(src_state* s, real v)
{
	if (s->out_n < s->out_cap) s->out[s->out_n] = (float) v;
	s->out_n++;
}

static void sr_inc(int* p) { if (++(*p) >= SRC_BUFFER_SIZE) (*p) -= SRC_BUFFER_SIZE; }
static void sr_dec(int* p) { if (--(*p) < 0) (*p) += SRC_BUFFER_SIZE; }

/* dataEmpty, SampleRateConverter.h:295-416 */
static void src_data_empty(src_state* s)
{
	int end_ptr = s->fill_ptr - s->pad_size;
	if (end_ptr < 0) end_ptr += SRC_BUFFER_SIZE;
	if (end_ptr < s->empty_ptr) end_ptr += SRC_BUFFER_SIZE;

	if (s->ratio >= RC(1.0)) {
		while (s->empty_ptr < end_ptr) {
			real output = RC(0.0);
			if (!s->count_only) {
				real interpolation = (real) (s->time_register & SRC_M_MASK) / SRC_M_RANGE;
				int index = s->empty_ptr;
				for (unsigned fi = (s->time_register & SRC_L_MASK) >> SRC_M_BITS; fi < SRC_FILTER_LENGTH;
						sr_dec(&index), fi += s->filter_increment) {
					output += (s->buffer[index] * (s->h[fi] + (s->delta_h[fi] * interpolation)));
				}
				s->time_register = ~s->time_register;
				interpolation = (real) (s->time_register & SRC_M_MASK) / SRC_M_RANGE;
				index = s->empty_ptr;
				sr_inc(&index);
				for (unsigned fi = (s->time_register & SRC_L_MASK) >> SRC_M_BITS; fi < SRC_FILTER_LENGTH;
						sr_inc(&index), fi += s->filter_increment) {
					output += (s->buffer[index] * (s->h[fi] + (s->delta_h[fi] * interpolation)));
				}
				s->time_register = ~s->time_register;
			}
			src_emit(s, output);
			s->time_register += s->time_register_increment;
			s->empty_ptr += (int) ((s->time_register & SRC_N_MASK) >> SRC_FRACTION_BITS);
			if (s->empty_ptr >= SRC_BUFFER_SIZE) {
				s->empty_ptr -= SRC_BUFFER_SIZE;
				end_ptr -= SRC_BUFFER_SIZE;
			}
			s->time_register &= (~SRC_N_MASK);
		}
	} else {
		while (s->empty_ptr < end_ptr) {
			real output = RC(0.0);
			if (!s->count_only) {
				unsigned phase_index = (unsigned) R_RINT((s->time_register & SRC_FRACTION_MASK) * s->ratio);
				int index = s->empty_ptr;
				unsigned impulse_index;
				while ((impulse_index = (phase_index >> SRC_M_BITS)) < SRC_FILTER_LENGTH) {
					const real impulse = s->h[impulse_index] + (s->delta_h[impulse_index] *
							((real) (phase_index & SRC_M_MASK) / SRC_M_RANGE));
					output += s->buffer[index] * impulse;
					sr_dec(&index);
					phase_index += s->phase_increment;
				}
				phase_index = (unsigned) R_RINT((real) ((~s->time_register) & SRC_FRACTION_MASK) * s->ratio);
				index = s->empty_ptr;
				sr_inc(&index);
				while ((impulse_index = (phase_index >> SRC_M_BITS)) < SRC_FILTER_LENGTH) {
					const real impulse = s->h[impulse_index] + (s->delta_h[impulse_index] *
							((real) (phase_index & SRC_M_MASK) / SRC_M_RANGE));
					output += s->buffer[index] * impulse;
					sr_inc(&index);
					phase_index += s->phase_increment;
				}
			}
			src_emit(s, output);
			s->time_register += s->time_register_increment;
			s->empty_ptr += (int) ((s->time_register & SRC_N_MASK) >> SRC_FRACTION_BITS);
			if (s->empty_ptr >= SRC_BUFFER_SIZE) {
				s->empty_ptr -= SRC_BUFFER_SIZE;
				end_ptr -= SRC_BUFFER_SIZE;
			}
			s->time_register &= (~SRC_N_MASK);
		}
	}
}

/* dataFill, SampleRateConverter.h:268-282 */
static void src_data_fill(src_state* s, real v)
{
	s->buffer[s->fill_ptr] = v;
	sr_inc(&s->fill_ptr);
	if (++s->fill_counter >= s->fill_size) {
		src_data_empty(s);
		s->fill_counter = 0;
	}
}

/* flushBuffer, SampleRateConverter.h:462-471 */
static void src_flush(src_state* s)
{
	for (int i = 0; i < s->pad_size * 2; ++i) src_data_fill(s, RC(0.0));
	src_data_empty(s);
}

/* ------------------------------------------------------------------------- */
/* one-pole / two-pole helpers                                                */

typedef struct { real b0, b1, a1, x1, y1; } radiation_filter;   /* vtm/RadiationFilter.h:54-79 */
typedef struct { real b0, a1, y1; } reflection_filter;          /* vtm/ReflectionFilter.h:55-76 */
typedef struct { real b0, a1, gain, y1; } throat_filter;        /* vtm/Throat.h:52-85 */
typedef struct {                                                  /* vtm/BandpassFilter.h */
	real b0, a2, a1, x1, x2, y1, y2, prev_rate, prev_bw, prev_cf;
} bandpass_filter;

static void radiation_init(radiation_filter* f, real a) { f->b0 = a; f->b1 = -f->b0; f->a1 = -f->b0; f->x1 = f->y1 = RC(0.0); }
static real radiation_run(radiation_filter* f, real x)
{
	const real y = f->b0 * x + f->b1 * f->x1 - f->a1 * f->y1;
	f->x1 = x;
	f->y1 = y;
	return y;
}
static void reflection_init(reflection_filter* f, real a) { f->b0 = RC(1.0) - R_FABS(a); f->a1 = -a; f->y1 = RC(0.0); }
static real reflection_run(reflection_filter* f, real x)
{
	const real y = f->b0 * x - f->a1 * f->y1;
	f->y1 = y;
	return y;
}
static void throat_init(throat_filter* f, real rate, real cutoff, real gain)
{
	f->b0 = (cutoff * RC(2.0)) / rate;
	f->a1 = f->b0 - RC(1.0);
	f->gain = gain;
	f->y1 = RC(0.0);
}
static real throat_run(throat_filter* f, real x)
{
	const real y = f->b0 * x - f->a1 * f->y1;
	f->y1 = y;
	return y * f->gain;
}
/* BandpassFilter::update, vtm/BandpassFilter.h:91-110 */
static void bandpass_update(bandpass_filter* f, real rate, real bw, real cf)
{
	if (rate == f->prev_rate && bw == f->prev_bw && cf == f->prev_cf) return;
	f->prev_rate = rate;
	f->prev_bw = bw;
	f->prev_cf = cf;
	const real pi = RC(M_PI);
	const real T = RC(1.0) / rate;
	const real tan_value = R_TAN(pi * bw * T);
	const real cos_value = R_COS(RC(2.0) * pi * cf * T);
	f->a2 = (RC(1.0) - tan_value) / (RC(1.0) + tan_value);
	f->a1 = -(RC(1.0) + f->a2) * cos_value;
	f->b0 = RC(0.5) - RC(0.5) * f->a2;
}
/* BandpassFilter::filter, vtm/BandpassFilter.h:114-122 */
static real bandpass_run(bandpass_filter* f, real x)
{
	const real y = f->b0 * (x - f->x2) - f->a1 * f->y1 - f->a2 * f->y2;
	f->x2 = f->x1;
	f->x1 = x;
	f->y2 = f->y1;
	f->y1 = y;
	return y;
}

/* ------------------------------------------------------------------------- */
/* the tube model                                                             */

#define MAX_DELAY 8

enum { S1, S2, S3, S4, S5, S6, S7, S8, S9, S10, N_SECTIONS };
enum { N1, N2, N3, N4, N5, N6, N_NASAL };
#define MAX_SECTIONS 30 /* VocalTractModel4: 30 oropharynx + 18 nasal sections */
#define MAX_NASAL 18
enum { P_PITCH, P_GLOT_VOL, P_ASP_VOL, P_FRIC_VOL, P_FRIC_POS, P_FRIC_CF, P_FRIC_BW,
       P_R1, P_R2, P_R3, P_R4, P_R5, P_R6, P_R7, P_R8, P_VELUM };

typedef struct { real top[MAX_DELAY + 1], bottom[MAX_DELAY + 1]; } section;

typedef struct {
	/* configuration (loadConfiguration, VocalTractModel0.h:266-305) */
	real output_rate, tp, tn_min, tn_max, breathiness, length, temperature, loss_factor;
	real aperture_radius, mouth_coef, nose_coef, nasal_radius[N_NASAL], throat_cutoff, throat_vol, mix_offset;
	real radius_coef[8];
	int waveform, modulation, delay, layout;
	/* derived (initializeSynthesizer, VocalTractModel0.h:338-392) */
	int sample_rate;
	real damping, crossmix_factor, breathiness_factor;
	/* state */
	section oro[MAX_SECTIONS], nasal[MAX_NASAL];
	unsigned in_ptr, out_ptr;
	real oro_k[8], nasal_k[N_NASAL], alpha_l, alpha_r, alpha_u, tap[8];
	real cur[VTMO_N_PARAM];
	radiation_filter mouth_rad, nose_rad;
	reflection_filter mouth_refl, nose_refl;
	throat_filter throat;
	bandpass_filter bandpass;
	glottal_source glottal;
	double noise_seed; /* NoiseSource is double whatever TFloat is (NoiseSource.h:52-54) */
	real noise_x1;
	src_state src;
	double* taps; /* optional debug taps for the current step: u, sig, thr, fir, lpnoise, pos0, pos1, x */
} vtm_model;

static real junction2(real left_radius, real right_radius)
{
	/* Junction2::configure, VocalTractModel2.h:214-218 == VocalTractModel0.h:488-490 */
	const real r0 = left_radius * left_radius;
	const real r1 = right_radius * right_radius;
	return (r0 - r1) / (r0 + r1);
}

/* loadConfiguration + initializeSynthesizer + initializeNasalCavity,
 * VocalTractModel0.h:266-305, :338-392, :457-470 (VocalTractModel2.h:335-376, :413-467, :534-543) */
static int model_init(vtm_model* m, const vtmo_config* c, int count_only)
{
	memset(m, 0, sizeof(*m));
	if (c->section_delay < 1 || c->section_delay > MAX_DELAY) return -1;
	m->delay = c->section_delay;
	m->layout = c->layout;
	if (m->layout != 0 && m->layout != 1) return -1;
	m->output_rate = c->output_rate;
	m->waveform = c->waveform;
	m->tp = c->glottal_pulse_tp;
	m->tn_min = c->glottal_pulse_tn_min;
	m->tn_max = c->glottal_pulse_tn_max;
	m->breathiness = c->breathiness;
	m->length = (real) c->vocal_tract_length_offset + (real) c->vocal_tract_length;
	if (m->length < RC(3.0)) m->length = RC(3.0);
	else if (m->length > RC(30.0)) m->length = RC(30.0);
	m->temperature = c->temperature;
	m->loss_factor = c->loss_factor;
	m->mouth_coef = c->mouth_coefficient;
	m->nose_coef = c->nose_coefficient;
	m->throat_cutoff = c->throat_cutoff;
	m->throat_vol = c->throat_volume;
	m->modulation = c->noise_modulation;
	m->mix_offset = c->mix_offset;
	m->aperture_radius = (real) c->aperture_radius * (real) c->global_radius_coef;
	m->nasal_radius[0] = RC(0.0);
	for (int i = 0; i < 5; ++i) m->nasal_radius[i + 1] = (real) c->nasal_radius[i] * (real) c->global_nasal_radius_coef;
	for (int i = 0; i < 8; ++i) m->radius_coef[i] = (real) c->radius_coef[i] * (real) c->global_radius_coef;

	/* reset(): VocalTractModel2.h:380-404 (inPtr 0, outPtr 1; D=1 is VocalTractModel0's cur/prev pair) */
	m->in_ptr = 0;
	m->out_ptr = 1;

	const real speed = RC(331.4) + (RC(0.6) * m->temperature); /* Util::speedOfSound, VTMUtil.h:104-110 */
	/* TOTAL_SECTIONS is 10 for VocalTractModel0/2 and 30 for VocalTractModel4 (VocalTractModel4.h:467) */
	m->sample_rate = (int) ((speed * ((m->layout ? MAX_SECTIONS : N_SECTIONS) * m->delay) * RC(100.0)) / m->length);
	const real nyquist = (real) ((float) m->sample_rate / 2.0f); /* int / float -> float arithmetic, VocalTractModel0.h:345 */
	m->breathiness_factor = m->breathiness / RC(100.0);
	m->crossmix_factor = RC(1.0) / amplitude60dB(m->mix_offset);
	m->damping = RC(1.0) - (m->loss_factor / RC(100.0));

	if (!count_only) {
		glottal_init(&m->glottal, m->waveform, (real) m->sample_rate, m->tp, m->tn_min, m->tn_max);
	}
	const real mouth_ap = (nyquist - m->mouth_coef) / nyquist;
	radiation_init(&m->mouth_rad, mouth_ap);
	reflection_init(&m->mouth_refl, mouth_ap);
	const real nose_ap = (nyquist - m->nose_coef) / nyquist;
	radiation_init(&m->nose_rad, nose_ap);
	reflection_init(&m->nose_refl, nose_ap);

	for (int i = N2; i < N6; ++i) m->nasal_k[i] = junction2(m->nasal_radius[i], m->nasal_radius[i + 1]);
	m->nasal_k[N6] = junction2(m->nasal_radius[N6], m->aperture_radius);

	throat_init(&m->throat, (real) m->sample_rate, m->throat_cutoff, amplitude60dB(m->throat_vol));
	src_init(&m->src, (real) m->sample_rate, m->output_rate, count_only);
	m->bandpass.prev_rate = m->bandpass.prev_bw = m->bandpass.prev_cf = -RC(1.0);
	m->noise_seed = 0.7892347; /* NoiseSource.h:32-34 */
	return 0;
}

/* setAllParameters, VocalTractModel0.h:698-716 */
static void model_set_parameters(vtm_model* m, const float* p)
{
	for (int i = P_PITCH; i <= P_FRIC_BW; ++i) m->cur[i] = p[i];
	for (int i = P_R1; i <= P_R8; ++i) {
		const real r = (real) p[i] * m->radius_coef[i - P_R1]; /* float * TFloat */
		m->cur[i] = (r < RC(0.01)) ? RC(0.01) : r; /* std::max(r, 0.01) */
	}
	m->cur[P_VELUM] = p[P_VELUM];
}

/* calculateTubeCoefficients, VocalTractModel0.h:484-512 */
static void model_tube_coefficients(vtm_model* m)
{
	for (int i = 0; i < 7; ++i) m->oro_k[i] = junction2(m->cur[P_R1 + i], m->cur[P_R1 + i + 1]);
	m->oro_k[7] = junction2(m->cur[P_R8], m->aperture_radius);
	const real r1_2 = m->cur[P_R4] * m->cur[P_R4];
	const real r0_2 = r1_2;
	const real r2_2 = m->cur[P_VELUM] * m->cur[P_VELUM];
	const real sum = RC(2.0) / (r0_2 + r1_2 + r2_2);
	m->alpha_l = sum * r0_2;
	m->alpha_r = sum * r1_2;
	m->alpha_u = sum * r2_2;
	const real rb = m->nasal_radius[N2] * m->nasal_radius[N2];
	m->nasal_k[N1] = (r2_2 - rb) / (r2_2 + rb);
}

/* setFricationTaps, VocalTractModel0.h:524-552 */
static void model_frication_taps(vtm_model* m)
{
	const real amp = amplitude60dB(m->cur[P_FRIC_VOL]);
	const int ip = (int) m->cur[P_FRIC_POS];
	const real complement = m->cur[P_FRIC_POS] - ip;
	const real remainder = RC(1.0) - complement;
	for (int i = 0; i < 8; ++i) {
		if (i == ip) {
			m->tap[i] = remainder * amp;
			if ((i + 1) < 8) m->tap[++i] = complement * amp;
		} else {
			m->tap[i] = RC(0.0);
		}
	}
}

static void propagate_junction(vtm_model* m, section* l, real k, section* r, real fric)
{
	/* propagateJunction(Junction2), VocalTractModel2.h:255-259 == VocalTractModel0.h:576-592 */
	const real delta = k * (l->top[m->out_ptr] - r->bottom[m->out_ptr]);
	r->top[m->in_ptr] = (l->top[m->out_ptr] + delta) * m->damping + fric;
	l->bottom[m->in_ptr] = (r->bottom[m->out_ptr] + delta) * m->damping;
}

/* vocalTract, VocalTractModel0.h:565-661 / VocalTractModel2.h:626-669 */
static real model_vocal_tract(vtm_model* m, real input, real frication)
{
	/* Section::movePointers, VocalTractModel2.h:241-248 */
	m->in_ptr = m->out_ptr;
	m->out_ptr = (m->out_ptr == (unsigned) m->delay) ? 0 : m->out_ptr + 1;
	const unsigned in = m->in_ptr, out = m->out_ptr;
	section* o = m->oro;
	section* n = m->nasal;
	const real d = m->damping;

	o[S1].top[in] = o[S1].bottom[out] * d + input;
	/* S1-S2: VocalTractModel0 adds no frication term here; x + 0.0 is exact */
	{
		const real delta = m->oro_k[0] * (o[S1].top[out] - o[S2].bottom[out]);
		o[S2].top[in] = (o[S1].top[out] + delta) * d;
		o[S1].bottom[in] = (o[S2].bottom[out] + delta) * d;
	}
	for (int i = S2, j = 1, k = 0; i < S4; ++i, ++j, ++k) {
		propagate_junction(m, &o[i], m->oro_k[j], &o[i + 1], m->tap[k] * frication);
	}
	{ /* 3-way junction, VocalTractModel0.h:595-604 */
		const real jp = (m->alpha_l * o[S4].top[out]) + (m->alpha_r * o[S5].bottom[out]) + (m->alpha_u * n[N1].bottom[out]);
		o[S4].bottom[in] = (jp - o[S4].top[out]) * d;
		o[S5].top[in] = ((jp - o[S5].bottom[out]) * d) + (m->tap[2] * frication);
		n[N1].top[in] = (jp - n[N1].bottom[out]) * d;
	}
	propagate_junction(m, &o[S5], m->oro_k[3], &o[S6], m->tap[3] * frication);
	/* pure delay with damping, VocalTractModel0.h:616-620 */
	o[S7].top[in] = (o[S6].top[out] * d) + (m->tap[4] * frication);
	o[S6].bottom[in] = o[S7].bottom[out] * d;
	for (int i = S7, j = 4, k = 5; i < S10; ++i, ++j, ++k) {
		propagate_junction(m, &o[i], m->oro_k[j], &o[i + 1], m->tap[k] * frication);
	}
	o[S10].bottom[in] = d * reflection_run(&m->mouth_refl, m->oro_k[7] * o[S10].top[out]);
	real output = radiation_run(&m->mouth_rad, (RC(1.0) + m->oro_k[7]) * o[S10].top[out]);

	for (int i = N1; i < N6; ++i) {
		const real delta = m->nasal_k[i] * (n[i].top[out] - n[i + 1].bottom[out]);
		n[i + 1].top[in] = (n[i].top[out] + delta) * d;
		n[i].bottom[in] = (n[i + 1].bottom[out] + delta) * d;
	}
	n[N6].bottom[in] = d * reflection_run(&m->nose_refl, m->nasal_k[N6] * n[N6].top[out]);
	output += radiation_run(&m->nose_rad, (RC(1.0) + m->nasal_k[N6]) * n[N6].top[out]);
	return output;
}

/* Simple copy between sections of one region, VocalTractModel4.h:296-300 */
static void propagate_copy(vtm_model* m, section* l, section* r)
{
	r->top[m->in_ptr] = l->top[m->out_ptr];
	l->bottom[m->in_ptr] = r->bottom[m->out_ptr];
}

/* Delay with damping and frication, VocalTractModel4.h:301-305 (== VocalTractModel2.h:251-254) */
static void propagate_damped(vtm_model* m, section* l, section* r, real fric)
{
	r->top[m->in_ptr] = l->top[m->out_ptr] * m->damping + fric;
	l->bottom[m->in_ptr] = r->bottom[m->out_ptr] * m->damping;
}

/* vocalTract of VocalTractModel4 (VocalTractModel4.h:671-745): 30 oropharynx + 18 nasal sections,
 * scattering only at the region boundaries, plain copies inside a region. */
static real model_vocal_tract4(vtm_model* m, real input, real frication)
{
	m->in_ptr = m->out_ptr;
	m->out_ptr = (m->out_ptr == (unsigned) m->delay) ? 0 : m->out_ptr + 1;
	const unsigned in = m->in_ptr, out = m->out_ptr;
	section* o = m->oro; /* o[i] = S(i+1) */
	section* n = m->nasal;
	const real d = m->damping;
	const real* k = m->oro_k; /* J1..J8 */
	const real* t = m->tap;   /* FC1..FC8 */

	o[0].top[in] = o[0].bottom[out] * d + input;
	propagate_copy(m, &o[0], &o[1]);
	propagate_copy(m, &o[1], &o[2]);
	propagate_junction(m, &o[2], k[0], &o[3], RC(0.0));
	propagate_copy(m, &o[3], &o[4]);
	propagate_junction(m, &o[4], k[1], &o[5], t[0] * frication);
	propagate_copy(m, &o[5], &o[6]);
	propagate_copy(m, &o[6], &o[7]);
	propagate_copy(m, &o[7], &o[8]);
	propagate_junction(m, &o[8], k[2], &o[9], t[1] * frication);
	propagate_copy(m, &o[9], &o[10]);
	propagate_copy(m, &o[10], &o[11]);
	{ /* 3-way junction S12 / S13 / N1 */
		const real jp = m->alpha_l * o[11].top[out] + m->alpha_r * o[12].bottom[out] + m->alpha_u * n[0].bottom[out];
		o[11].bottom[in] = (jp - o[11].top[out]) * d;
		o[12].top[in] = (jp - o[12].bottom[out]) * d + t[2] * frication;
		n[0].top[in] = (jp - n[0].bottom[out]) * d;
	}
	propagate_copy(m, &o[12], &o[13]);
	propagate_copy(m, &o[13], &o[14]);
	propagate_junction(m, &o[14], k[3], &o[15], t[3] * frication);
	propagate_copy(m, &o[15], &o[16]);
	propagate_copy(m, &o[16], &o[17]);
	propagate_damped(m, &o[17], &o[18], t[4] * frication);
	propagate_copy(m, &o[18], &o[19]);
	propagate_copy(m, &o[19], &o[20]);
	propagate_junction(m, &o[20], k[4], &o[21], t[5] * frication);
	propagate_copy(m, &o[21], &o[22]);
	propagate_copy(m, &o[22], &o[23]);
	propagate_copy(m, &o[23], &o[24]);
	propagate_junction(m, &o[24], k[5], &o[25], t[6] * frication);
	propagate_copy(m, &o[25], &o[26]);
	propagate_junction(m, &o[26], k[6], &o[27], t[7] * frication);
	propagate_copy(m, &o[27], &o[28]);
	propagate_copy(m, &o[28], &o[29]);
	o[29].bottom[in] = d * reflection_run(&m->mouth_refl, k[7] * o[29].top[out]);
	real output = radiation_run(&m->mouth_rad, (RC(1.0) + k[7]) * o[29].top[out]);

	for (int g = 0; g < 6; ++g) { /* nasal regions of three sections, junction after each but the last */
		propagate_copy(m, &n[3 * g], &n[3 * g + 1]);
		propagate_copy(m, &n[3 * g + 1], &n[3 * g + 2]);
		if (g < 5) propagate_junction(m, &n[3 * g + 2], m->nasal_k[g], &n[3 * g + 3], RC(0.0));
	}
	n[17].bottom[in] = d * reflection_run(&m->nose_refl, m->nasal_k[5] * n[17].top[out]);
	output += radiation_run(&m->nose_rad, (RC(1.0) + m->nasal_k[5]) * n[17].top[out]);
	return output;
}

/* execSynthesisStep, VocalTractModel0.h:396-445; returns the sample handed to the SRC */
static real model_step(vtm_model* m)
{
	const real f0 = frequency(m->cur[P_PITCH]);
	const real ax = amplitude60dB(m->cur[P_GLOT_VOL]);
	const real ah1 = amplitude60dB(m->cur[P_ASP_VOL]);
	model_tube_coefficients(m);
	model_frication_taps(m);
	bandpass_update(&m->bandpass, (real) m->sample_rate, m->cur[P_FRIC_BW], m->cur[P_FRIC_CF]);

	/* NoiseSource::getSample NoiseSource.h:40-44; NoiseFilter::filter NoiseFilter.h:63-68 */
	const double product = m->noise_seed * 377.0;
	m->noise_seed = product - (int) product;
	const real white = (real) (m->noise_seed - 0.5); /* getSample() returns double, NoiseFilter<TFloat>::filter takes TFloat */
	const real lp_noise = white + m->noise_x1;
	m->noise_x1 = white;

	if (m->waveform == 0) glottal_setup(&m->glottal, ax);
	m->glottal.tap_pos = m->taps ? m->taps + 5 : NULL;
	real pulse = glottal_sample(&m->glottal, f0);
	if (m->taps) { m->taps[3] = pulse; m->taps[4] = lp_noise; }
	const real pulsed_noise = lp_noise * pulse;
	pulse = ax * ((pulse * (RC(1.0) - m->breathiness_factor)) + (pulsed_noise * m->breathiness_factor));

	real signal;
	if (m->modulation) {
		real crossmix = ax * m->crossmix_factor;
		crossmix = (crossmix < RC(1.0)) ? crossmix : RC(1.0);
		signal = (pulsed_noise * crossmix) + (lp_noise * (RC(1.0) - crossmix));
	} else {
		signal = lp_noise;
	}
	const real fric = bandpass_run(&m->bandpass, signal);
	if (m->taps) { m->taps[0] = (pulse + (ah1 * signal)) * RC(0.125); m->taps[1] = signal; m->taps[2] = pulse * RC(0.125); }
	signal = m->layout ? model_vocal_tract4(m, ((pulse + (ah1 * signal)) * RC(0.125)), fric)
	                   : model_vocal_tract(m, ((pulse + (ah1 * signal)) * RC(0.125)), fric);
	signal += throat_run(&m->throat, pulse * RC(0.125));
	if (m->taps) m->taps[7] = signal;
	return signal;
}


/* ------------------------------------------------------------------------- */
/* VocalTractModel5 (vtm/VocalTractModel5.h): 30 + 21 sections, flow scattering junctions, Rosenberg B
 * source, pole-zero radiation impedance at mouth and nose, Butterworth noise / source filters, glottal
 * loss, differentiated output.  Not yet served by the device path (SURVEY.md 8f rank 4): restated and
 * pinned here so that the kernel can be built against it. */

typedef struct { real b0, a1, x1, y1; } butter1;                 /* vtm/Butterworth1LowpassFilter.h */
typedef struct { real b0, b1, a1, a2, x1, x2, y1, y2; } butter2f; /* vtm/Butterworth2LowpassFilter.h */

/* Butterworth1LowPassFilter::update, Butterworth1LowpassFilter.h:63-76 */
static void butter1_design(butter1* f, real rate, real cutoff)
{
	const real pi = RC(M_PI);
	const real wcT = RC(2.0) * R_TAN(pi * cutoff / rate);
	const real c1 = RC(1.0) / (wcT + RC(2.0));
	f->b0 = c1 * wcT;
	f->a1 = c1 * (wcT - RC(2.0));
	f->x1 = f->y1 = RC(0.0);
}
static real butter1_run(butter1* f, real x) /* :80-86 */
{
	const real y = f->b0 * (x + f->x1) - f->a1 * f->y1;
	f->x1 = x;
	f->y1 = y;
	return y;
}
/* Butterworth2LowPassFilter::update, Butterworth2LowpassFilter.h:88-107 */
static void butter2f_design(butter2f* f, real rate, real cutoff)
{
	const real pi = RC(M_PI);
	const real wcT = RC(2.0) * R_TAN(pi * cutoff / rate);
	const real wc2T2 = wcT * wcT;
	const real c1 = RC(2.0) * R_SQRT(RC(2.0)) * wcT;
	const real c2 = RC(1.0) / (wc2T2 + c1 + RC(4.0));
	f->b0 = c2 * wc2T2;
	f->b1 = RC(2.0) * f->b0;
	f->a1 = c2 * (RC(2.0) * wc2T2 - RC(8.0));
	f->a2 = c2 * (wc2T2 - c1 + RC(4.0));
	f->x1 = f->x2 = f->y1 = f->y2 = RC(0.0);
}
static real butter2f_run(butter2f* f, real x) /* :111-120 */
{
	const real y = f->b0 * (x + f->x2) + f->b1 * f->x1 - f->a1 * f->y1 - f->a2 * f->y2;
	f->x2 = f->x1;
	f->x1 = x;
	f->y2 = f->y1;
	f->y1 = y;
	return y;
}

/* PoleZeroRadiationImpedance, vtm/PoleZeroRadiationImpedance.h */
typedef struct { real period, in1, outT1, outR1, cT1, cT2, cT3, cR1, cR2, cR3, prev_radius; } radiation_impedance;

static void radimp_init(radiation_impedance* r, real rate)
{
	memset(r, 0, sizeof(*r));
	r->prev_radius = -RC(1.0);
	r->period = RC(1.0) / rate;
}
static void radimp_update(radiation_impedance* r, real radius) /* :139-172 */
{
	if (radius == r->prev_radius) return;
	r->prev_radius = radius;
	const real transition_radius = RC(0.5e-2);
	real rr = radius;
	if (rr < transition_radius) rr = transition_radius;
	const real trans_freq = RC(62.3371) / rr + RC(320.204);
	const real cos_wt = R_COS(RC(2.0 * M_PI) * trans_freq * r->period);
	const real qa = RC(2.0) * cos_wt;
	const real qb = -RC(2.0) * (cos_wt + RC(1.0));
	const real qc = cos_wt + RC(1.0);
	const real delta = qb * qb - RC(4.0) * qa * qc;
	real a = (-qb - R_SQRT(delta)) / (RC(2.0) * qa);
	const real b = RC(2.0) * a - RC(1.0);
	if (radius < transition_radius) a *= RC(40391.2) * (radius * radius);
	const real coef = RC(1.0) / (a + RC(1.0));
	const real a_plus_b = a + b;
	r->cT1 = a_plus_b * coef;
	r->cT2 = RC(2.0) * coef;
	r->cT3 = -RC(2.0) * b * coef;
	r->cR1 = a_plus_b * coef;
	r->cR2 = (a - RC(1.0)) * coef;
	r->cR3 = (b - a) * coef;
}
static void radimp_process(radiation_impedance* r, real in, real* outT, real* outR) /* :176-184 */
{
	*outT = r->cT1 * r->outT1 + r->cT2 * in + r->cT3 * r->in1;
	*outR = r->cR1 * r->outR1 + r->cR2 * in + r->cR3 * r->in1;
	r->in1 = in;
	r->outT1 = *outT;
	r->outR1 = *outR;
}

enum { V5_SECTIONS = 30, V5_NASAL = 21 };

typedef struct {
	/* configuration (loadConfiguration, VocalTractModel5.h:375-421) */
	real output_rate, tp, tn_min, tn_max, breathiness, length, temperature, loss_factor, mix_offset;
	real nasal_radius[7], radius_coef[8];
	real glottal_noise_cutoff, frication_noise_cutoff, frication_factor, min_glottal_loss, max_glottal_loss, glottal_lowpass_cutoff;
	int waveform, modulation, bypass, constant_mouth;
	real mouth_impedance_radius;
	/* derived (initializeSynthesizer, :455-521) */
	real sample_rate, damping, crossmix_factor, breathiness_factor;
	/* state */
	real otop[V5_SECTIONS][2], obot[V5_SECTIONS][2], ntop[V5_NASAL][2], nbot[V5_NASAL][2];
	unsigned in_ptr, out_ptr;
	real oro_k[7], nasal_k[6], velum_l, velum_r, velum_u;
	real cur[VTMO_N_PARAM];
	radiation_impedance mouth, nose;
	bandpass_filter bandpass;
	butter1 glottal_noise, glottal_filter;
	butter2f frication_noise;
	double noise_seed;
	/* RosenbergBGlottalSource, vtm/RosenbergBGlottalSource.h */
	real rb_tn_min, rb_tn_max, rb_t1, rb_t2, rb_next_t2, rb_prev_amp, rb_t;
	float diff_x1, diff_x2; /* DifferenceFilter<float>, vtm/DifferenceFilter.h */
	src_state src;
	float* final_out;
	size_t final_cap, final_n;
} vtm5_model;

static int v5_init(vtm5_model* m, const vtmo5_config* c, int count_only)
{
	memset(m, 0, sizeof(*m));
	m->output_rate = c->output_rate;
	m->waveform = c->waveform;
	m->tp = c->glottal_pulse_tp;
	m->tn_min = c->glottal_pulse_tn_min;
	m->tn_max = c->glottal_pulse_tn_max;
	m->breathiness = c->breathiness;
	m->length = (real) c->vocal_tract_length_offset + (real) c->vocal_tract_length;
	if (m->length < RC(3.0)) m->length = RC(3.0);       /* MIN_VOCAL_TRACT_LENGTH, VocalTractModel5.h:67 */
	else if (m->length > RC(30.0)) m->length = RC(30.0);
	m->temperature = c->temperature;
	m->loss_factor = c->loss_factor;
	m->modulation = c->noise_modulation;
	m->mix_offset = c->mix_offset;
	m->nasal_radius[0] = RC(0.0);
	for (int i = 0; i < 6; ++i) m->nasal_radius[i + 1] = (real) c->nasal_radius[i] * (real) c->global_nasal_radius_coef;
	for (int i = 0; i < 8; ++i) m->radius_coef[i] = (real) c->radius_coef[i] * (real) c->global_radius_coef;
	m->glottal_noise_cutoff = c->glottal_noise_cutoff;
	m->frication_noise_cutoff = c->frication_noise_cutoff;
	m->frication_factor = c->frication_factor;
	m->min_glottal_loss = c->min_glottal_loss;
	m->max_glottal_loss = c->max_glottal_loss;
	m->glottal_lowpass_cutoff = c->glottal_lowpass_cutoff;
	m->bypass = c->bypass;
	m->constant_mouth = c->constant_radius_mouth_impedance;
	m->mouth_impedance_radius = c->mouth_impedance_radius;

	m->in_ptr = 0; /* reset(), :436-437 */
	m->out_ptr = 1;

	const real speed = RC(331.4) + (RC(0.6) * m->temperature);
	m->sample_rate = (speed * (V5_SECTIONS * 1) * RC(100.0)) / m->length; /* TFloat, not truncated (:463) */
	m->breathiness_factor = m->breathiness / RC(100.0);
	m->crossmix_factor = RC(1.0) / amplitude60dB(m->mix_offset);
	m->damping = RC(1.0) - (m->loss_factor / RC(100.0));

	/* RosenbergBGlottalSource ctor, RosenbergBGlottalSource.h:66-96 */
	m->rb_tn_min = m->tn_min / RC(100.0);
	m->rb_tn_max = m->tn_max / RC(100.0);
	m->rb_t1 = m->tp / RC(100.0);
	m->rb_t2 = m->rb_t1 + m->rb_tn_max;
	m->rb_next_t2 = m->rb_t2;
	m->rb_prev_amp = -RC(1.0);
	m->rb_t = RC(0.0);

	radimp_init(&m->mouth, m->sample_rate);
	if (m->constant_mouth) radimp_update(&m->mouth, m->mouth_impedance_radius * (real) 1.0e-2f);
	radimp_init(&m->nose, m->sample_rate);
	/* initializeNasalCavity, :577-587 */
	for (int i = 1; i < 6; ++i) m->nasal_k[i] = junction2(m->nasal_radius[i], m->nasal_radius[i + 1]);
	{
		const real r = R_SQRT(RC(0.5) * m->nasal_radius[6] * m->nasal_radius[6]);
		radimp_update(&m->nose, r * (real) 1.0e-2f);
	}
	src_init(&m->src, m->sample_rate, m->output_rate, count_only);
	m->bandpass.prev_rate = m->bandpass.prev_bw = m->bandpass.prev_cf = -RC(1.0);
	butter1_design(&m->glottal_noise, m->sample_rate, m->glottal_noise_cutoff);
	butter2f_design(&m->frication_noise, m->sample_rate, m->frication_noise_cutoff);
	butter1_design(&m->glottal_filter, m->sample_rate, m->glottal_lowpass_cutoff);
	m->noise_seed = 0.7892347;
	return 0;
}

static void v5_set_parameters(vtm5_model* m, const float* p) /* setAllParameters, :768-786 */
{
	for (int i = P_PITCH; i <= P_FRIC_BW; ++i) m->cur[i] = p[i];
	for (int i = P_R1; i <= P_R8; ++i) {
		const real r = (real) p[i] * m->radius_coef[i - P_R1];
		m->cur[i] = (r < RC(0.01)) ? RC(0.01) : r;
	}
	m->cur[P_VELUM] = p[P_VELUM];
}

/* propagate / propagateJunction, VocalTractModel5.h:285-303 */
static void v5_copy(vtm5_model* m, real (*top)[2], real (*bot)[2], int l)
{
	top[l + 1][m->in_ptr] = top[l][m->out_ptr] * m->damping;
	bot[l][m->in_ptr] = bot[l + 1][m->out_ptr] * m->damping;
}
static void v5_junction(vtm5_model* m, real (*top)[2], real (*bot)[2], int l, real k)
{
	const real delta = k * (top[l][m->out_ptr] + bot[l + 1][m->out_ptr]);
	top[l + 1][m->in_ptr] = (top[l][m->out_ptr] - delta) * m->damping;
	bot[l][m->in_ptr] = (bot[l + 1][m->out_ptr] + delta) * m->damping;
}

/* vocalTract, VocalTractModel5.h:632-730 */
static real v5_vocal_tract(vtm5_model* m, real input, real frication, real glottal_loss)
{
	m->in_ptr = m->out_ptr;
	m->out_ptr = (m->out_ptr == 1u) ? 0 : m->out_ptr + 1;
	const unsigned in = m->in_ptr, out = m->out_ptr;
	real (*ot)[2] = m->otop;
	real (*ob)[2] = m->obot;
	real (*nt)[2] = m->ntop;
	real (*nb)[2] = m->nbot;

	ot[0][in] = ob[0][out] * glottal_loss + input;
	/* junction after section index: J1 after S3 (2), J2 after S5 (4), J3 after S9 (8), 3-way after S12 (11),
	 * J4 after S15 (14), J5 after S21 (20), J6 after S25 (24), J7 after S27 (26); plain damped links elsewhere */
	static const signed char oro_kind[V5_SECTIONS - 1] = {
		-1, -1, 0, -1, 1, -1, -1, -1, 2, -1, -1, 99, -1, -1, 3, -1, -1, -1, -1, -1, 4, -1, -1, -1, 5, -1, 6, -1, -1};
	for (int l = 0; l < V5_SECTIONS - 1; ++l) {
		const int kind = oro_kind[l];
		if (kind == -1) {
			v5_copy(m, ot, ob, l);
		} else if (kind == 99) { /* Junction3, :296-303 */
			const real partial = ot[11][out] + ob[12][out] + nb[0][out];
			ob[11][in] = (ob[12][out] + nb[0][out] + m->velum_l * partial) * m->damping;
			ot[12][in] = (ot[11][out] + nb[0][out] + m->velum_r * partial) * m->damping;
			nt[0][in] = (ot[11][out] + ob[12][out] + m->velum_u * partial) * m->damping;
		} else {
			v5_junction(m, ot, ob, l, m->oro_k[kind]);
		}
	}
	real mouth_flow;
	radimp_process(&m->mouth, ot[29][out], &mouth_flow, &ob[29][in]);
	ob[29][in] *= m->damping;

	for (int l = 0; l < V5_NASAL - 1; ++l) {
		if (l % 3 == 2) v5_junction(m, nt, nb, l, m->nasal_k[l / 3]); /* NJ1..NJ6 after N3, N6, ..., N18 */
		else v5_copy(m, nt, nb, l);
	}
	real nasal_flow;
	radimp_process(&m->nose, nt[20][out], &nasal_flow, &nb[20][in]);
	nb[20][in] *= m->damping;

	/* frication noise (:716-726) */
	const real fric_offset = (27 - 5) * (m->cur[P_FRIC_POS] / RC(7.0 - 0.0));
	/* THE PRODUCT'S RULE, not the reference's: the reference indexes oropharynx_[5 + (int) offset] unguarded, which is
	 * defined only while that section is one of the 30 (S1..S30: -6 < offset < 25, the cast truncates towards zero).
	 * Outside -- decided on the floating offset, before a cast that is itself undefined beyond the range of int --
	 * nothing is injected.  Inside, this is the reference's arithmetic unchanged. */
	if (fric_offset > RC(-6.0) && fric_offset < RC(25.0)) {
		const int fric_int = (int) fric_offset;
		const real fric_right = fric_offset - fric_int;
		const real fric_left = RC(1.0) - fric_right;
		const real fric_amp = amplitude60dB(m->cur[P_FRIC_VOL]);
		const real fric_value = fric_amp * frication;
		ot[5 + fric_int][in] += fric_value * fric_left;
		if (5 + fric_int < 27) ot[5 + fric_int + 1][in] += fric_value * fric_right;
	}

	return mouth_flow + nasal_flow;
}

/* RosenbergBGlottalSource::setup / getSample, RosenbergBGlottalSource.h:109-147 */
static real v5_glottal_sample(vtm5_model* m, real amplitude, real frequency)
{
	if (m->waveform == 0) {
		if (!(m->rb_tn_min == m->rb_tn_max || amplitude == m->rb_prev_amp)) {
			m->rb_next_t2 = m->rb_t1 + m->rb_tn_max - amplitude * (m->rb_tn_max - m->rb_tn_min);
			m->rb_prev_amp = amplitude;
		}
	}
	real value;
	if (m->waveform == 0) {
		if (m->rb_t < m->rb_t1) {
			const real x = m->rb_t / m->rb_t1;
			value = (x * x) * (RC(3.0) - RC(2.0) * x);
		} else if (m->rb_t < m->rb_t2) {
			const real x = (m->rb_t - m->rb_t1) / (m->rb_t2 - m->rb_t1);
			value = RC(1.0) - x * x;
		} else {
			value = RC(0.0);
		}
	} else {
		value = R_SIN(m->rb_t * RC(2.0 * M_PI));
	}
	const real dt = frequency / m->sample_rate;
	m->rb_t += dt;
	if (m->rb_t > RC(1.0)) {
		m->rb_t -= RC(1.0);
		m->rb_t2 = m->rb_next_t2;
	}
	return value;
}

/* execSynthesisStep, VocalTractModel5.h:523-571 (interactive_ == false) */
static real v5_step(vtm5_model* m)
{
	const real f0 = frequency(m->cur[P_PITCH]);
	const real glot_amp = amplitude60dB(m->cur[P_GLOT_VOL]);
	const real asp_amp = amplitude60dB(m->cur[P_ASP_VOL]);
	/* calculateTubeCoefficients, :600-620 */
	for (int i = 0; i < 7; ++i) m->oro_k[i] = junction2(m->cur[P_R1 + i], m->cur[P_R1 + i + 1]);
	if (!m->constant_mouth) radimp_update(&m->mouth, m->cur[P_R8] * (real) 1.0e-2f);
	{ /* Junction3::configure(R4, R4, velum), :266-276 */
		const real r0_2 = m->cur[P_R4] * m->cur[P_R4];
		const real r1_2 = m->cur[P_R4] * m->cur[P_R4];
		const real r2_2 = m->cur[P_VELUM] * m->cur[P_VELUM];
		const real c = RC(1.0) / (r0_2 + r1_2 + r2_2);
		m->velum_l = c * (r0_2 - r1_2 - r2_2);
		m->velum_r = c * (r1_2 - r0_2 - r2_2);
		m->velum_u = c * (r2_2 - r0_2 - r1_2);
	}
	m->nasal_k[0] = junction2(m->cur[P_VELUM], m->nasal_radius[1]);
	bandpass_update(&m->bandpass, m->sample_rate, m->cur[P_FRIC_BW], m->cur[P_FRIC_CF]);

	const double product = m->noise_seed * 377.0;
	m->noise_seed = product - (int) product;
	const real noise_sample = (real) (m->noise_seed - 0.5);
	const real glottal_noise = butter1_run(&m->glottal_noise, noise_sample);
	const real pulse = butter1_run(&m->glottal_filter, v5_glottal_sample(m, glot_amp, f0));
	const real pulsed_noise = glottal_noise * pulse;
	const real noisy_pulse = glot_amp * (pulse * (RC(1.0) - m->breathiness_factor) + pulsed_noise * m->breathiness_factor);
	real frication_noise = butter2f_run(&m->frication_noise, noise_sample);
	if (m->modulation) {
		real crossmix = glot_amp * m->crossmix_factor;
		crossmix = (crossmix < RC(1.0)) ? crossmix : RC(1.0);
		frication_noise = frication_noise * (noisy_pulse * crossmix + (RC(1.0) - crossmix));
	}
	real signal;
	if (m->bypass == 1) {
		signal = noisy_pulse + asp_amp * frication_noise;
	} else {
		const real min_loss = RC(1.0) - glot_amp * (m->min_glottal_loss / RC(100.0));
		const real max_loss = RC(1.0) - glot_amp * (m->max_glottal_loss / RC(100.0));
		const real glottal_loss = min_loss + (max_loss - min_loss) * pulse;
		signal = v5_vocal_tract(m, noisy_pulse + asp_amp * frication_noise,
				m->frication_factor * bandpass_run(&m->bandpass, frication_noise), glottal_loss);
	}
	return signal;
}

/* the sample-rate converter's sink (:497-513): differentiate and scale unless bypassed */
static void v5_drain(vtm5_model* m, size_t from)
{
	for (size_t i = from; i < m->src.out_n && i < m->src.out_cap; ++i) {
		float v = m->src.out[i];
		if (m->bypass != 1) {
			const float y = v - m->diff_x2; /* DifferenceFilter<float>::filter */
			m->diff_x2 = m->diff_x1;
			m->diff_x1 = v;
			v = (float) (y * m->output_rate);
		}
		if (m->final_n < m->final_cap) m->final_out[m->final_n] = v;
		m->final_n++;
	}
}

size_t PUB(vtmo5_run)(const vtmo5_config* cfg, double control_rate, const float* params, size_t n_frames,
		float* out, size_t cap, int* sample_rate_milli)
{
	vtm5_model* m = (vtm5_model*) malloc(sizeof(vtm5_model));
	if (!m) return (size_t) -1;
	v5_init(m, cfg, 0);
	if (sample_rate_milli) *sample_rate_milli = (int) (m->sample_rate * RC(1000.0));
	/* raw resampler output goes to a scratch buffer, then through the sink */
	const size_t raw_cap = cap + 64;
	float* raw = (float*) malloc(sizeof(float) * (raw_cap ? raw_cap : 1));
	if (!raw) { free(m); return (size_t) -1; }
	m->src.out = raw;
	m->src.out_cap = raw_cap;
	m->final_out = out;
	m->final_cap = cap;
	if (n_frames > 0) {
		const unsigned control_steps = (unsigned) rint((double) m->sample_rate / control_rate);
		const float coef = 1.0f / control_steps;
		float cur[VTMO_N_PARAM], delta[VTMO_N_PARAM];
		for (size_t i = 1; i <= n_frames; ++i) {
			const float* p0 = params + (i - 1) * VTMO_N_PARAM;
			const float* p1 = params + ((i < n_frames) ? i : n_frames - 1) * VTMO_N_PARAM;
			for (int j = 0; j < VTMO_N_PARAM; ++j) {
				cur[j] = p0[j];
				delta[j] = (p1[j] - cur[j]) * coef;
			}
			for (unsigned j = 0; j < control_steps; ++j) {
				v5_set_parameters(m, cur);
				src_data_fill(&m->src, v5_step(m));
				for (int k = 0; k < VTMO_N_PARAM; ++k) cur[k] += delta[k];
			}
		}
	}
	src_flush(&m->src);
	v5_drain(m, 0);
	const size_t n = m->src.out_n;
	free(raw);
	free(m);
	return n;
}

/* ------------------------------------------------------------------------- */
/* entry points of this precision (dispatched by vtm_oracle.c)                */

int PUB(vtmo_derive)(const vtmo_config* cfg, double control_rate, vtmo_derived* out)
{
	vtm_model* m = (vtm_model*) malloc(sizeof(vtm_model));
	if (!m) return -1;
	if (model_init(m, cfg, 0) != 0) { free(m); return -1; }
	out->sample_rate = m->sample_rate;
	out->control_steps = (unsigned) rint((double) m->sample_rate / control_rate);
	out->fir_taps = m->glottal.taps;
	out->table_div1 = m->glottal.div1;
	out->table_div2 = m->glottal.div2;
	out->tn_delta = m->glottal.tn_delta;
	out->time_register_increment = m->src.time_register_increment;
	out->phase_increment = m->src.phase_increment;
	out->pad_size = m->src.pad_size;
	out->upsampling = m->src.ratio >= 1.0;
	free(m);
	return 0;
}

size_t PUB(vtmo_run)(const vtmo_config* cfg, double control_rate, const float* params, size_t n_frames,
		float* out, size_t cap, double* internal_signal, int count_only, double* taps)
{
	vtm_model* m = (vtm_model*) malloc(sizeof(vtm_model));
	if (!m) return (size_t) -1;
	if (model_init(m, cfg, count_only) != 0) { free(m); return (size_t) -1; }
	m->src.out = out;
	m->src.out_cap = cap;

	/* Controller::synthesize, vtm_control_model/Controller.cpp:277-313.  The
	 * appended copy of the last frame (:283) is expressed by clamping the index. */
	if (n_frames > 0) {
		const unsigned control_steps = (unsigned) rint((double) m->sample_rate / control_rate);
		const float coef = 1.0f / control_steps;
		float cur[VTMO_N_PARAM], delta[VTMO_N_PARAM];
		size_t step = 0;
		for (size_t i = 1; i <= n_frames; ++i) {
			const float* p0 = params + (i - 1) * VTMO_N_PARAM;
			const float* p1 = params + ((i < n_frames) ? i : n_frames - 1) * VTMO_N_PARAM;
			for (int j = 0; j < VTMO_N_PARAM && !count_only; ++j) {
				cur[j] = p0[j];
				delta[j] = (p1[j] - cur[j]) * coef;
			}
			for (unsigned j = 0; j < control_steps; ++j, ++step) {
				if (count_only) {
					src_data_fill(&m->src, RC(0.0));
				} else {
					model_set_parameters(m, cur);
					m->taps = taps ? taps + step * 8 : NULL;
					const real s = model_step(m);
					if (internal_signal) internal_signal[step] = s;
					src_data_fill(&m->src, s);
				}
				for (int k = 0; k < VTMO_N_PARAM && !count_only; ++k) cur[k] += delta[k];
			}
		}
	}
	src_flush(&m->src); /* finishSynthesis, VocalTractModel0.h:720-723 */
	const size_t n = m->src.out_n;
	free(m);
	return n;
}

