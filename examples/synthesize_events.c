/* Plain-C use of include/gama_vtm.h without linking HIP: EVENT LISTS in from host memory, 16-bit samples out, for a ragged
 * batch in one call -- what Controller::synthesizePhoneticStringToFile does for one utterance.  Three utterances of one,
 * two and no chunks (the /c chunks of the phonetic string, each an event list of its own) are described by two offset
 * tables; the frames are generated on the device and come back only because this program asks for them (the reference's
 * vtmParamFile).
 *
 * Build (from the repo root):
 *   gcc -std=c99 -Wall -Wextra -Werror -O2 -Iinclude examples/synthesize_events.c -Lgama_tts_amd/lib -lgama_vtm \
 *       -Wl,-rpath,$PWD/gama_tts_amd/lib -o /tmp/synthesize_events
 * Without an MI355X the program prints the layout (design-only plan) and stops at the synthesis call with
 * GVTM_ERR_NO_DEVICE (there is no CPU path). */
#include <math.h>
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

static gvtm_track_config male_tracks(void)
{
	/* 0_male/vtm_control_model.txt as Controller.cpp:70-81 sets its EventList up */
	gvtm_track_config t = {0};
	t.control_period_ms = 4;
	t.macro_intonation = t.micro_intonation = t.intonation_drift = t.smooth_intonation = 1;
	t.initial_pitch = -20.0;
	t.mean_pitch = -4.0 + -12.0;
	t.drift_deviation = 4.0;
	t.drift_sample_rate = 250.0;
	t.drift_lowpass_cutoff = 4.0;
	return t;
}

/* an event at time_ms that sets every parameter (vowel: open tube; pause: closed glottis) and no special parameter */
static gvtm_event posture(int time_ms, int vowel)
{
	const double open[GVTM_N_PARAM] = {-2.0, 60.0, 0.0, 0.0, 5.5, 2500.0, 500.0, 0.8, 0.89, 0.99, 0.81, 0.76, 1.05, 1.23, 0.01, 0.1};
	const double rest[GVTM_N_PARAM] = {-6.0, 0.0, 0.0, 0.0, 5.5, 2500.0, 500.0, 0.8, 0.89, 0.99, 0.81, 0.76, 1.05, 1.23, 0.01, 0.1};
	gvtm_event e = {0};
	int k;
	e.time_ms = time_ms;
	for (k = 0; k < GVTM_N_PARAM; ++k) {
		e.param[k] = vowel ? open[k] : rest[k];
		e.special[k] = HUGE_VAL; /* Event::EMPTY_PARAMETER */
	}
	return e;
}

#define BATCH 3
#define N_CHUNKS 3
#define N_EVENTS 9

int main(void)
{
	/* utterance 0: one chunk of 400 ms; utterance 1: two chunks of 200 and 120 ms; utterance 2: none */
	const int times[N_EVENTS] = {0, 100, 300, 400, 0, 100, 200, 0, 120};
	const int vowel[N_EVENTS] = {0, 1, 1, 0, 0, 1, 0, 1, 0};
	const int64_t chunk_offsets[N_CHUNKS + 1] = {0, 4, 7, 9};
	const int64_t utt_chunks[BATCH + 1] = {0, 1, 3, 3};
	gvtm_event events[N_EVENTS];
	gvtm_config cfg = male_voice();
	gvtm_track_config tracks = male_tracks();
	gvtm_plan* plan = NULL;
	int64_t frame_offsets[BATCH + 1], sample_offsets[BATCH + 1], counts[BATCH];
	float peaks[BATCH], scales[BATCH];
	size_t capacity, b;
	int k, rc, device = gvtm_device_count() > 0 ? 0 : GVTM_DEVICE_NONE;

	for (k = 0; k < N_EVENTS; ++k) events[k] = posture(times[k], vowel[k]);
	rc = gvtm_plan_create(&cfg, 250.0, device, &plan);
	if (rc == GVTM_OK) rc = gvtm_plan_set_voice_tracks(plan, &tracks, 1);
	if (rc != GVTM_OK) {
		fprintf(stderr, "plan: %s (%s)\n", gvtm_status_string(rc), gvtm_last_error());
		return 1;
	}
	/* the layout needs no device: the host walks the lists */
	capacity = gvtm_events_packed_layout(plan, events, chunk_offsets, utt_chunks, NULL, BATCH, frame_offsets, sample_offsets);
	if (capacity == (size_t) -1) {
		fprintf(stderr, "layout: %s\n", gvtm_last_error());
		return 1;
	}
	for (b = 0; b < BATCH; ++b) {
		printf("utterance %zu: %lld chunks -> %lld frames -> samples at offset %lld\n", b, (long long) (utt_chunks[b + 1] - utt_chunks[b]),
				(long long) (frame_offsets[b + 1] - frame_offsets[b]), (long long) sample_offsets[b]);
	}
	printf("packed output: %zu samples, %lld frames\n", capacity, (long long) frame_offsets[BATCH]);
	{
		const size_t total_frames = (size_t) frame_offsets[BATCH];
		float* frames = malloc(sizeof(float) * (total_frames ? total_frames : 1) * GVTM_N_PARAM);
		int16_t* pcm = malloc(sizeof(int16_t) * (capacity ? capacity : 1));
		if (!frames || !pcm) return 1;
		rc = gvtm_synthesize_events_packed_host_pcm16(plan, events, chunk_offsets, utt_chunks, NULL, BATCH, pcm, capacity, NULL, NULL, frames,
				total_frames, counts, peaks, scales, NULL);
		if (rc != GVTM_OK) {
			printf("synthesis: %s (%s)\n", gvtm_status_string(rc), gvtm_last_error());
		} else {
			for (b = 0; b < BATCH; ++b) {
				printf("utterance %zu: %lld samples at [%lld, %lld), peak %g scaled by %g", b, (long long) counts[b], (long long) sample_offsets[b],
						(long long) (sample_offsets[b] + counts[b]), peaks[b], scales[b]);
				if (frame_offsets[b + 1] > frame_offsets[b]) printf(", first frame's pitch %g", frames[frame_offsets[b] * GVTM_N_PARAM]);
				printf("\n");
				if (sample_offsets[b] + counts[b] > sample_offsets[b + 1]) rc = GVTM_ERR_INVALID_ARGUMENT;
			}
		}
		free(frames); free(pcm);
	}
	gvtm_plan_destroy(plan);
	return rc == GVTM_OK || rc == GVTM_ERR_NO_DEVICE ? 0 : 1;
}
