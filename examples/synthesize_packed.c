/* Plain-C use of include/gama_vtm.h: a RAGGED batch through the packed host entry.  Three utterances of different
 * lengths go in back to back (no padding to the longest), described by a table of frame offsets, and their 16-bit samples
 * come out back to back, described by a table of sample offsets: what crosses PCIe and what the device stages is the
 * utterances, not the rectangle around them.
 *
 * Build (from the repo root):
 *   gcc -std=c99 -Wall -Wextra -Werror -O2 -Iinclude examples/synthesize_packed.c -Lgama_tts_amd/lib -lgama_vtm \
 *       -Wl,-rpath,$PWD/gama_tts_amd/lib -o /tmp/synthesize_packed
 * Without an MI355X the program prints the layout (design-only plan) and stops at the synthesis call with
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

#define BATCH 3

int main(void)
{
	/* 0.16 s, 1 s and 28 ms at 250 frames per second: padded to the longest, 58 % of the rectangle would be padding */
	const int64_t frame_offsets[BATCH + 1] = {0, 40, 290, 297};
	const float frame[GVTM_N_PARAM] = {-12.0f, 60.0f, 0.0f, 0.0f, 5.5f, 2500.0f, 500.0f,
	                                   0.8f, 0.89f, 0.99f, 0.81f, 0.76f, 1.05f, 1.23f, 0.01f, 0.1f};
	gvtm_config cfg = male_voice();
	gvtm_plan* plan = NULL;
	int64_t sample_offsets[BATCH + 1], counts[BATCH];
	float peaks[BATCH], scales[BATCH];
	size_t capacity, b, f, total_frames = (size_t) frame_offsets[BATCH];
	int k, rc, device = gvtm_device_count() > 0 ? 0 : GVTM_DEVICE_NONE;

	rc = gvtm_plan_create(&cfg, 250.0, device, &plan);
	if (rc != GVTM_OK) {
		fprintf(stderr, "plan: %s (%s)\n", gvtm_status_string(rc), gvtm_last_error());
		return 1;
	}
	/* the layout needs no device: where each utterance starts, and what the output buffer must hold */
	capacity = gvtm_packed_sample_offsets(plan, frame_offsets, NULL, BATCH, sample_offsets);
	if (capacity == (size_t) -1) {
		fprintf(stderr, "layout: %s\n", gvtm_last_error());
		return 1;
	}
	for (b = 0; b < BATCH; ++b) {
		printf("utterance %zu: %lld frames -> %zu samples at offset %lld\n", b, (long long) (frame_offsets[b + 1] - frame_offsets[b]),
				gvtm_output_count(plan, (size_t) (frame_offsets[b + 1] - frame_offsets[b])), (long long) sample_offsets[b]);
	}
	printf("packed output: %zu samples (every start a multiple of %d)\n", capacity, GVTM_PACKED_ALIGN);
	{
		float* frames = malloc(sizeof(float) * (total_frames ? total_frames : 1) * GVTM_N_PARAM);
		int16_t* pcm = malloc(sizeof(int16_t) * (capacity ? capacity : 1));
		if (!frames || !pcm) return 1;
		for (f = 0; f < total_frames; ++f) {
			for (k = 0; k < GVTM_N_PARAM; ++k) frames[f * GVTM_N_PARAM + k] = frame[k];
		}
		rc = gvtm_synthesize_packed_host_pcm16(plan, frames, frame_offsets, NULL, BATCH, pcm, capacity, NULL, counts, peaks, scales);
		if (rc != GVTM_OK) {
			printf("synthesis: %s (%s)\n", gvtm_status_string(rc), gvtm_last_error());
		} else {
			for (b = 0; b < BATCH; ++b) {
				int16_t top = 0;
				int64_t i;
				for (i = 0; i < counts[b]; ++i) {
					const int16_t v = pcm[sample_offsets[b] + i];
					if (v > top) top = v;
					if (v < 0 && -v > top) top = (int16_t) -v;
				}
				printf("utterance %zu: %lld samples at [%lld, %lld), peak %g scaled by %g -> |pcm| up to %d\n", b, (long long) counts[b],
						(long long) sample_offsets[b], (long long) (sample_offsets[b] + counts[b]), peaks[b], scales[b], (int) top);
				if (sample_offsets[b] + counts[b] > sample_offsets[b + 1]) rc = GVTM_ERR_INVALID_ARGUMENT;
			}
		}
		free(frames); free(pcm);
	}
	gvtm_plan_destroy(plan);
	return rc == GVTM_OK || rc == GVTM_ERR_NO_DEVICE ? 0 : 1;
}
