/* Plain-C use of include/gama_vtm.h without linking HIP: PARAMETER-MODIFICATION GESTURES on one base track -- what the
 * editor's parameter-modification window leaves in its modified list when the user drags a parameter while the utterance
 * plays, and what its "synthesize to file" then speaks.  Three gestures: r3 is opened by 0.3 from 80 ms on (ADD), the
 * frication volume is scaled to 60 % around the middle and back (MULTIPLY), and a second ADD on r3 starts later and takes
 * the rest of the utterance over from the first.  The rule runs on the host and needs no device; the synthesis does.
 *
 * Build (from the repo root):
 *   gcc -std=c99 -Wall -Wextra -Werror -O2 -Iinclude examples/synthesize_modified.c -Lgama_tts_amd/lib -lgama_vtm \
 *       -Wl,-rpath,$PWD/gama_tts_amd/lib -o /tmp/synthesize_modified
 * Without an MI355X the program prints the modified frames (design-only plan) and stops at the synthesis call with
 * GVTM_ERR_NO_DEVICE (there is no CPU path). */
#include <stdio.h>
#include <stdlib.h>

#include "gama_vtm.h"

static gvtm_config male_voice(void)
{
	/* data/voice/english/0_male: vtm.txt + variant/male.txt, model = 0 */
	gvtm_config c = {0};
	const double nasal[5] = {1.35, 1.96, 1.91, 1.3, 0.73};
	int i;
	c.output_rate = 44100.0;
	c.waveform = 0;
	c.noise_modulation = 1;
	c.glottal_pulse_tp = 40.0;
	c.glottal_pulse_tn_min = 24.0;
	c.glottal_pulse_tn_max = 24.0;
	c.breathiness = 0.5;
	c.vocal_tract_length_offset = 0.0;
	c.vocal_tract_length = 17.5;
	c.temperature = 32.0;
	c.loss_factor = 0.8;
	c.mouth_coefficient = 5000.0;
	c.nose_coefficient = 5000.0;
	c.throat_cutoff = 1500.0;
	c.throat_volume = 6.0;
	c.mix_offset = 48.0;
	c.global_radius_coef = 1.0;
	c.global_nasal_radius_coef = 1.0;
	c.aperture_radius = 3.05;
	for (i = 0; i < 5; ++i) c.nasal_radius[i] = nasal[i];
	for (i = 0; i < 8; ++i) c.radius_coef[i] = 1.0;
	c.section_delay = 1;
	c.precision = GVTM_PRECISION_F64;
	c.tube_layout = GVTM_TUBE_10_6;
	return c;
}

#define FRAMES 100 /* 400 ms at 250 Hz */
#define N_GESTURES 3
#define N_POINTS 6
#define R3 9
#define FRIC_VOL 3

int main(void)
{
	/* a vowel with some frication under it, the same in every frame */
	const float posture[GVTM_N_PARAM] = {-2.0f, 60.0f, 0.0f, 12.0f, 5.5f, 2500.0f, 500.0f, 0.8f, 0.89f, 0.99f, 0.81f, 0.76f, 1.05f, 1.23f, 0.01f, 0.1f};
	const int32_t gestures[N_GESTURES][2] = {{R3, GVTM_MODIFICATION_ADD}, {FRIC_VOL, GVTM_MODIFICATION_MULTIPLY}, {R3, GVTM_MODIFICATION_ADD}};
	const int64_t gesture_offsets[N_GESTURES + 1] = {0, 2, 5, 6};
	int32_t point_steps[N_POINTS];
	const float point_values[N_POINTS] = {0.0f, 0.3f, 1.0f, 0.6f, 1.0f, -0.2f};
	const int point_ms[N_POINTS] = {60, 80, 100, 180, 260, 300};
	const int touched[2] = {R3, FRIC_VOL};
	static float base[FRAMES][GVTM_N_PARAM], modified[FRAMES][GVTM_N_PARAM];
	gvtm_config cfg = male_voice();
	gvtm_plan* plan = NULL;
	gvtm_info info;
	int32_t status = -1;
	int64_t n, count = 0;
	float peak = 0.0f;
	float* audio;
	size_t stride;
	int f, k, j, rc, device = gvtm_device_count() > 0 ? 0 : GVTM_DEVICE_NONE;

	for (f = 0; f < FRAMES; ++f) {
		for (k = 0; k < GVTM_N_PARAM; ++k) base[f][k] = posture[k];
	}
	rc = gvtm_plan_create(&cfg, 250.0, device, &plan);
	if (rc == GVTM_OK) rc = gvtm_plan_info(plan, &info);
	if (rc != GVTM_OK) {
		fprintf(stderr, "plan: %s (%s)\n", gvtm_status_string(rc), gvtm_last_error());
		return 1;
	}
	/* a gesture's points lie at internal steps: control_steps of them per frame of 1000 / control_rate ms */
	for (j = 0; j < N_POINTS; ++j) point_steps[j] = (int32_t) ((double) point_ms[j] * info.control_rate / 1000.0 * info.control_steps);
	n = gvtm_modification_filter_length(plan, 0);
	printf("internal rate %g Hz, %u steps per frame, the 20 ms filter holds %lld samples\n", info.internal_rate_hz, info.control_steps, (long long) n);
	rc = gvtm_modification_apply_host(plan, 0, &base[0][0], FRAMES, &gestures[0][0], gesture_offsets, N_GESTURES, point_steps, point_values,
			&modified[0][0], &status);
	if (rc != GVTM_OK || status != 0) {
		fprintf(stderr, "apply: %s (%s), status %d\n", gvtm_status_string(rc), gvtm_last_error(), (int) status);
		return 1;
	}
	for (j = 0; j < 2; ++j) {
		int first = -1, last = -1;
		k = touched[j];
		for (f = 0; f < FRAMES; ++f) {
			if (modified[f][k] != base[f][k]) {
				if (first < 0) first = f;
				last = f;
			}
		}
		if (first < 0) {
			printf("parameter %d: no frame modified\n", k);
		} else {
			printf("parameter %d: first modified frame %d: %g -> %g, last %d: %g -> %g\n", k, first, base[first][k], modified[first][k], last,
					base[last][k], modified[last][k]);
		}
	}
	stride = gvtm_output_count(plan, FRAMES);
	audio = malloc(sizeof(float) * (stride ? stride : 1));
	if (!audio) return 1;
	rc = gvtm_synthesize_batch_host(plan, &modified[0][0], NULL, 1, FRAMES, audio, stride, &count, &peak);
	if (rc != GVTM_OK) {
		printf("synthesis: %s (%s)\n", gvtm_status_string(rc), gvtm_last_error());
	} else {
		printf("%lld samples, peak %g\n", (long long) count, peak);
	}
	free(audio);
	gvtm_plan_destroy(plan);
	return rc == GVTM_OK || rc == GVTM_ERR_NO_DEVICE ? 0 : 1;
}
