/*
 * gama_vtm.h — C ABI of the MI355X-native batched vocal-tract-model synthesizer.
 *
 * This is the drop-in boundary for GamaTTS's VTM hot path.  Plain C: pointers,
 * sizes and error codes only (no C++/torch types).  The library behind it
 * (libgama_vtm.so) is HIP for gfx950; there is no CPU fallback — every entry
 * point that needs the device fails with GVTM_ERR_NO_DEVICE / GVTM_ERR_HIP
 * when it is missing.
 *
 * Reference interfaces each entry replaces (paths under gama_tts/src/):
 *
 *   gvtm_plan_create            VocalTractModel0/2/4 constructor: loadConfiguration +
 *                               initializeSynthesizer (vtm/VocalTractModel0.h:255-305, :338-392;
 *                               vtm/VocalTractModel2.h:322-376, :413-467; vtm/VocalTractModel4.h:370-515)
 *                               for a whole batch
 *   gvtm_plan_create_model5     VocalTractModel5 constructor (vtm/VocalTractModel5.h:375-421, :455-521); synthesis
 *                               then replaces its execSynthesisStep / vocalTract (:523-579, :632-730)
 *   gvtm_plan_create_model5_float
 *                               the same constructor and steps of VocalTractModel5<float,1>, the class the factory has no
 *                               number for
 *   gvtm_plan_info              VocalTractModel::internalSampleRate/outputSampleRate
 *                               (vtm/VocalTractModel.h:51-52) and the controlSteps of
 *                               Controller::synthesize (vtm_control_model/Controller.cpp:286)
 *   gvtm_output_count           outputBuffer().size() after finishSynthesis()
 *                               (vtm/VocalTractModel.h:58, vtm/SampleRateConverter.h:462-471)
 *   gvtm_synthesize_batch_*     Controller::synthesize + VocalTractModel::setAllParameters /
 *                               execSynthesisStep / finishSynthesis for B utterances
 *                               (vtm_control_model/Controller.cpp:277-313,
 *                               vtm/VocalTractModel0.h:396-445, :698-723)
 *   gvtm_stream_*               the same three calls as a STATEFUL object: what VocalTractModel keeps between
 *                               execSynthesisStep() calls (vtm/VocalTractModel0.h:221-252, :396-445), reset() (:309-326)
 *                               and finishSynthesis() (:720-723), so that an utterance can be handed over in pieces
 *                               (long tracks; the editor's interactive polling, InteractiveAudio.cpp:141-185)
 *   gvtm_synthesize_batch_host_pcm16
 *                               the path as `gama_tts vtm` ends it: Controller::synthesizeToFile's int16 samples
 *                               (Controller.cpp:236-252, :325-340; WAVEFileWriter.cpp:122-125)
 *   gvtm_synthesize_events_device
 *                               EventList::generateOutput (vtm_control_model/EventList.cpp:930-1091) followed by
 *                               Controller::synthesize in one call: event lists in, samples out
 *   gvtm_plan_set_voice_tracks / gvtm_generate_tracks_voices_device / gvtm_synthesize_events_voices_device
 *                               the same for a batch that mixes voices: one EventList set-up per voice
 *                               (vtm_control_model/Controller.cpp:70-81)
 *   gvtm_generate_tracks_chunks_device / gvtm_synthesize_events_chunks_device
 *                               the same for utterances of several event lists: the loop over the /c chunks of
 *                               Controller::getParametersFromPhoneticString (vtm_control_model/Controller.cpp:141-154)
 *   gvtm_synthesize_events_packed_host*
 *                               Controller::synthesizePhoneticStringToFile (vtm_control_model/Controller.cpp:194-200 with
 *                               :141-154) for a ragged batch: event lists in from host memory, int16 samples out
 *   gvtm_rules_create / gvtm_generate_events_device / gvtm_synthesize_postures_device / gvtm_rules_apply_host
 *                               EventList::generateEventList and applyRule (vtm_control_model/EventList.cpp:435-676) for a
 *                               batch: posture sequences in, event lists (resp. samples) out
 *   gvtm_apply_modifications_device / gvtm_synthesize_modified_device / gvtm_modification_apply_host
 *                               the editor's parameter-modification window: what Processor::process leaves in its modified
 *                               parameter list (gama_tts_editor/src/ParameterModificationSynthesis.cpp:117-194), then
 *                               Controller::synthesizeToFile on it (ParameterModificationWindow.cpp:200-231, 281-322)
 *   gvtm_synthesize_targets_device / gvtm_targets_apply_host
 *                               the editor's interactive window: targets for the 16 parameters, each smoothed by a 50 ms
 *                               MovingAverageFilter<float> on every internal step, then execSynthesisStep()
 *                               (gama_tts_editor/src/interactive/InteractiveAudio.cpp:164-186);
 *                               gvtm_stream_push_targets: the same as a session, targets arriving push by push
 *                               (reference model 5, which the window constructs: gvtm_stream_push_targets_model5);
 *                               gvtm_synthesize_targets_voices_device: the same for a batch that mixes voices
 *                               (reference model 5: gvtm_synthesize_targets_model5_voices_device), and as a session
 *                               gvtm_stream_push_targets_voices (gvtm_stream_push_targets_model5_voices)
 *   gvtm_analysis_* / gvtm_analyze_spectrum_device
 *                               the same window's analysis view: AnalysisWindow::showData and setupWindow
 *                               (gama_tts_editor/src/interactive/AnalysisWindow.cpp:189-361) on each full ring of 65 536
 *                               output samples (InteractiveAudio.cpp:146-158, 192-205), for a batch of audio rows
 *   gvtm_stream_listen / gvtm_stream_take_spectra
 *                               that ring itself, kept on the device for every utterance of a stream: each push leaves
 *                               the views of the rings it completed ("Streams that listen")
 *   gvtm_plan_create_voices / gvtm_plan_create_model5_voices / gvtm_plan_create_model5_float_voices /
 *   gvtm_synthesize_voices_*
 *                               the same for a batch that mixes voices: one VocalTractModel per GamaTTS voice variant
 *                               (data/voice/english/0_male/vtm.txt resp. 5_male/vtm.txt + variant/{male,female,
 *                               large_child,small_child,baby}.txt, merged by Controller.cpp:48-49), all of them in one launch
 *   gvtm_normalize_batch_device Controller::writeOutputToBuffer / writeOutputToFile scaling,
 *                               Util::calculateOutputScale (Controller.cpp:315-340,
 *                               vtm/VTMUtil.cpp:48-67, WAVEFileWriter.cpp:122-125)
 *
 * The GamaTTS plugin entry points GAMA_TTS_construct_vocal_tract_model /
 * GAMA_TTS_destruct_vocal_tract_model (vtm/VocalTractModelPlugin.cpp:40-50) are
 * exported by libgama_vtm_plugin.so, which is a thin C++ shim over this ABI
 * (see include/gama_vtm_plugin.h and INTEGRATION.md).
 */
#ifndef GAMA_VTM_H_
#define GAMA_VTM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the libraries are built with -fvisibility=hidden: these entry points are their exports */
#endif

#define GVTM_N_PARAM 16 /* pitch, glotVol, aspVol, fricVol, fricPos, fricCF, fricBW, r1..r8, velum
                           (vtm/VocalTractModel0.h:160-178) */

typedef enum gvtm_status {
	GVTM_OK = 0,
	GVTM_ERR_INVALID_ARGUMENT = 1, /* null pointer, bad size, bad configuration value */
	GVTM_ERR_NO_DEVICE = 2,        /* no HIP device / device index out of range */
	GVTM_ERR_HIP = 3,              /* a HIP runtime call failed (see gvtm_last_error) */
	GVTM_ERR_UNSUPPORTED = 4,      /* valid for the reference but not implemented on the device (e.g. a workgroup shape
	                                  whose buffers do not fit LDS) */
	GVTM_ERR_OUT_OF_MEMORY = 5
} gvtm_status;

/* Arithmetic the device path computes in. */
typedef enum gvtm_precision {
	GVTM_PRECISION_F64 = 0,  /* everything in fp64, like VocalTractModel0<double> */
	GVTM_PRECISION_MIXED = 1, /* fp64 sources, tube and filters; fp32 sample-rate converter (tables, window, MACs) */
	GVTM_PRECISION_F32 = 2    /* everything in fp32, like VocalTractModel0<float> (reference model 1) and
	                             VocalTractModel2<float,D>: design tables and constants computed in float too, every
	                             rounding reproduced — the output is bit-identical to the reference's FLOAT model
	                             (which itself differs from its double model by several percent of peak after a
	                             few seconds: oscillator phase, 47 instead of 49 FIR taps) */
} gvtm_precision;

/* Tube topology. */
typedef enum gvtm_tube_layout {
	GVTM_TUBE_10_6 = 0,  /* 10 oropharynx + 6 nasal sections: VocalTractModel0 / VocalTractModel2 (models 0, 2, 3) */
	GVTM_TUBE_30_18 = 1  /* 30 + 18 sections, scattering at region boundaries only: VocalTractModel4 (model 4,
	                        vtm/VocalTractModel4.h); SectionDelay 1 */
} gvtm_tube_layout;

/* The configuration keys VocalTractModel0/2::loadConfiguration reads from the merged
 * vtm.txt + variant file (vtm/VocalTractModel0.h:266-305), as numbers. */
typedef struct gvtm_config {
	double output_rate;
	int32_t waveform; /* 0 pulse, 1 sine */
	int32_t noise_modulation;
	double glottal_pulse_tp;
	double glottal_pulse_tn_min;
	double glottal_pulse_tn_max;
	double breathiness;
	double vocal_tract_length_offset;
	double vocal_tract_length;
	double temperature;
	double loss_factor;
	double mouth_coefficient;
	double nose_coefficient;
	double throat_cutoff;
	double throat_volume;
	double mix_offset;
	double global_radius_coef;
	double global_nasal_radius_coef;
	double aperture_radius;
	double nasal_radius[5]; /* nasal_radius_1 .. nasal_radius_5 */
	double radius_coef[8];  /* radius_1_coef .. radius_8_coef */
	int32_t section_delay;  /* VocalTractModel2's SectionDelay; 1 == VocalTractModel0 (models 0/2), 3 == model 3 */
	int32_t precision;      /* gvtm_precision */
	int32_t tube_layout;    /* gvtm_tube_layout */
	int32_t reserved_;      /* must be 0 */
} gvtm_config;

typedef struct gvtm_info {
	int32_t internal_sample_rate; /* Hz, vtm/VocalTractModel0.h:344 */
	uint32_t control_steps;       /* internal steps per control frame, Controller.cpp:286 */
	double output_rate;
	double control_rate;
	int32_t fir_taps;                 /* glottal-source FIR, WavetableGlottalSourceFIRFilter.h:86 */
	uint32_t time_register_increment; /* SampleRateConverter.h:145 */
	uint32_t phase_increment;         /* SampleRateConverter.h:154 (0 when up-sampling) */
	int32_t pad_size;                 /* SampleRateConverter.h:158-160 */
	int32_t upsampling;
	int32_t device;
	int32_t precision;
	int32_t section_delay;
	int32_t model5;                   /* 1 for a plan made by gvtm_plan_create_model5 / _model5_voices / _model5_float / _model5_float_voices */
	int32_t reserved_;
	double internal_rate_hz;          /* the internal rate as the model holds it: an integer for models 0-4, not for
	                                     model 5 (vtm/VocalTractModel5.h:465 keeps it in TFloat) */
} gvtm_info;

/* The configuration keys VocalTractModel5::loadConfiguration reads (vtm/VocalTractModel5.h:375-421), as numbers:
 * reference model 5 — 30 + 21 sections with flow junctions, Rosenberg B glottal source, pole-zero radiation
 * impedance at mouth and nose, Butterworth noise/source filters, glottal loss, differentiated output.
 * The frication enters the section S6 + (int)(22 fricPos / 7) and its right neighbour (:716-726): for every position whose
 * section is one of S1..S30 (about -1.909 < fricPos < 7.954) a model 5 plan computes what the reference computes; for any
 * other position, where the reference indexes its array out of bounds, nothing is injected. */
typedef struct gvtm5_config {
	double output_rate;
	int32_t waveform;                         /* 0 pulse, 1 sine */
	int32_t noise_modulation;
	int32_t bypass;                           /* 1: the glottal signal goes straight to the resampler (:566-568) */
	int32_t constant_radius_mouth_impedance;  /* 0: the mouth impedance follows r8 every step */
	double glottal_pulse_tp;
	double glottal_pulse_tn_min;
	double glottal_pulse_tn_max;
	double breathiness;
	double vocal_tract_length_offset;
	double vocal_tract_length;
	double temperature;
	double loss_factor;
	double mix_offset;
	double global_radius_coef;
	double global_nasal_radius_coef;
	double nasal_radius[6];                   /* nasal_radius_2 .. nasal_radius_7 */
	double radius_coef[8];
	double glottal_noise_cutoff;
	double frication_noise_cutoff;
	double frication_factor;
	double min_glottal_loss;
	double max_glottal_loss;
	double glottal_lowpass_cutoff;
	double mouth_impedance_radius;            /* used when constant_radius_mouth_impedance != 0 */
	int32_t precision;                        /* GVTM_PRECISION_F64 for gvtm_plan_create_model5 / _model5_voices: the factory's
	                                             model 5 is VocalTractModel5<double,1> (vtm/VocalTractModel.cpp:47-48);
	                                             GVTM_PRECISION_F32 for gvtm_plan_create_model5_float / _model5_float_voices */
	int32_t reserved_;                        /* must be 0 */
} gvtm5_config;

typedef struct gvtm_plan gvtm_plan;

/* device index for a design-only plan: tables, info and output counts are available on a
 * machine without a GPU; every synthesis entry point returns GVTM_ERR_NO_DEVICE. */
#define GVTM_DEVICE_NONE (-1)

/* Design-time tables of a plan, for inspection/tests. */
typedef enum gvtm_table {
	GVTM_TABLE_FIR = 0,       /* fir_taps doubles */
	GVTM_TABLE_SRC_H = 1,     /* 3328 doubles */
	GVTM_TABLE_SRC_DH = 2,    /* 3328 doubles */
	GVTM_TABLE_WAVETABLE = 3  /* 512 doubles */
} gvtm_table;

const char* gvtm_status_string(int status);
/* Message of the last failing call on this thread ("" if none). */
const char* gvtm_last_error(void);
/* Number of HIP devices visible (0 when there is none or the runtime is unusable). */
int gvtm_device_count(void);

/* Validates the configuration, designs the tables on the host (fp64) and uploads them to
 * `device`.  control_rate is 1000 / control_period Hz (VTMControlModelConfiguration.cpp:41). */
int gvtm_plan_create(const gvtm_config* config, double control_rate, int device, gvtm_plan** plan_out);
/* The same for reference model 5 (VocalTractModel5 constructor: loadConfiguration + initializeSynthesizer,
 * vtm/VocalTractModel5.h:375-421, :455-521).  The plan is used with the same synthesis entry points;
 * gvtm_plan_table() serves the resampler tables only.  Refused (GVTM_ERR_INVALID_ARGUMENT), as the reference's constructors
 * refuse them: an internal rate below 50 kHz (vocal tract longer than ~21 cm, PoleZeroRadiationImpedance.h:116-119),
 * glottal pulse timings outside RosenbergBGlottalSource's checks, Butterworth cutoffs outside 1 Hz .. 0.48 of the internal
 * rate; and, a limit of this implementation, an output rate above 3x the internal rate. */
int gvtm_plan_create_model5(const gvtm5_config* config, double control_rate, int device, gvtm_plan** plan_out);
/* VocalTractModel5<float,1> (no factory number; oracle/ref_driver.cpp's "5f"): config->precision must be
 * GVTM_PRECISION_F32 (else GVTM_ERR_INVALID_ARGUMENT).  Everything else as gvtm_plan_create_model5: the same refusals, the
 * same synthesis, stream and events entry points, every constant designed in float as the class's constructors do and
 * every rounding of its steps reproduced, so the samples are bit-identical to that class's.  gvtm_plan_info reports
 * model5 = 1, precision = GVTM_PRECISION_F32 and the float class's internal_rate_hz; gvtm_plan_table serves the float
 * resampler tables (widened).  One voice per plan: the gvtm_synthesize_voices_* entries refuse it (GVTM_ERR_UNSUPPORTED);
 * gvtm_plan_create_model5_float_voices makes the float plans they take. */
int gvtm_plan_create_model5_float(const gvtm5_config* config, double control_rate, int device, gvtm_plan** plan_out);
void gvtm_plan_destroy(gvtm_plan* plan);
int gvtm_plan_info(const gvtm_plan* plan, gvtm_info* info_out);
/* Copies a design table into out[capacity]; returns the element count or a negative status. */
int gvtm_plan_table(const gvtm_plan* plan, int which, double* out, size_t capacity);

/* Samples finishSynthesis() leaves for an utterance of n_frames frames; (size_t)-1 for a null plan.  Includes the
 * reference converter's flush overrun (vtm/SampleRateConverter.h:298-308 with :462-471): on down-sampling plans
 * (reference models 3, 4, 5 at 44.1 / 48 kHz) about 0.4 % of the frame counts make flushBuffer()'s final dataEmpty()
 * convert one more lap of the 1024-sample ring (~750 extra samples computed from ring leftovers); the device
 * reproduces those samples, so such a count is LARGER than that of the next longer utterance. */
size_t gvtm_output_count(const gvtm_plan* plan, size_t n_frames);
/* max over n <= max_frames of gvtm_output_count(plan, n): the audio_stride that holds every utterance of a ragged
 * batch.  Equal to gvtm_output_count(plan, max_frames) on up-sampling plans. */
size_t gvtm_output_capacity(const gvtm_plan* plan, size_t max_frames);

/*
 * Batch synthesis, everything resident in device memory.
 *   d_params       [batch][max_frames][16] float32, reference frame order
 *   d_frame_counts [batch] int32 frames per utterance (<= max_frames), or NULL: all max_frames
 *   d_audio        [batch][audio_stride] float32, unscaled samples as in outputBuffer();
 *                  audio_stride >= gvtm_output_count(plan, max_frames) is required, gvtm_output_capacity(plan,
 *                  max_frames) holds every utterance of a ragged batch (samples beyond audio_stride are dropped,
 *                  d_out_counts still reports them); [count, audio_stride) of a row is left untouched
 *   d_out_counts   [batch] int64 samples per utterance, may be NULL
 *   d_maxabs       [batch] float32 max|x| per utterance, may be NULL
 *   hip_stream     hipStream_t (NULL = default stream); the call only enqueues work
 *                  (GVTM_PRECISION_F32 plans: the first call, and a later one with more frames than any before, also builds
 *                  and uploads the plan's noise-sample table for max_frames frames, 4 bytes per internal step, synchronously;
 *                  gvtm_plan_reserve(plan, max_frames) does that ahead of time, and every later call of up to that many
 *                  frames is then really enqueue-only)
 */
int gvtm_synthesize_batch_device(gvtm_plan* plan, const float* d_params, const int32_t* d_frame_counts,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int64_t* d_out_counts, float* d_maxabs, void* hip_stream);

/* Same with host buffers (H2D, kernel, D2H, synchronous).  frame_counts may be NULL.  A frame_counts[b] outside
 * [0, max_frames] fails that utterance only: out_counts[b] = -1, its row zeroed, the call still returns GVTM_OK
 * (gvtm_last_error() names the cause).  Rows are zero beyond their sample count.  The caller's current HIP device
 * is restored before returning (every entry point does). */
int gvtm_synthesize_batch_host(gvtm_plan* plan, const float* params, const int32_t* frame_counts,
		size_t batch, size_t max_frames, float* audio, size_t audio_stride,
		int64_t* out_counts, float* maxabs);

/* The same path ending where the reference's file writer ends (Controller::writeOutputToFile, Controller.cpp:325-340 with
 * WAVEFileWriter::writeSample, WAVEFileWriter.cpp:122-125): pcm[b][i] = round(x[b][i] * (0.95 / max|x[b]|) * 32767) as
 * int16, exactly the samples `gama_tts vtm` puts into its WAV file -- 2 bytes per sample cross PCIe instead of 4.
 *   pcm        [batch][pcm_stride] int16, rows zero beyond their sample count
 *   scales     [batch] the factor 0.95 / max|x| applied to each utterance (0 for silence), may be NULL
 *   maxabs     [batch] max|x| of the unscaled samples, may be NULL
 * Both host entries cut a batch of two or more machine-fulls (utterances per workgroup x compute units) into slices and
 * run   H2D frames(i+1) || kernel(i) [+ scaling(i)] || D2H samples(i-1)   on three streams.  The overlap is real when
 * the host buffers are page-locked (gvtm_host_alloc, hipHostMalloc, hipHostRegister); pageable buffers give the same
 * bytes, with the runtime staging the copies. */
int gvtm_synthesize_batch_host_pcm16(gvtm_plan* plan, const float* params, const int32_t* frame_counts,
		size_t batch, size_t max_frames, int16_t* pcm, size_t pcm_stride,
		int64_t* out_counts, float* maxabs, float* scales);

/* ---------------------------------------------------------------------------------------------
 * Several voices in one plan: a batch whose utterances are spoken by different voices (GamaTTS voice variants: male,
 * female, children, ...) synthesized in one launch.  Each voice is a gvtm_config of its own; voice v's utterances come out
 * bit for bit as a single-voice plan made from configs[v] synthesizes them, in every precision.
 */

/* configs[n_voices]: one model, several voices.  output_rate, section_delay, precision and tube_layout must be equal
 * across configs (else GVTM_ERR_INVALID_ARGUMENT); every other key may differ per voice.  The design runs per voice; the
 * device holds one constants block and one glottal wavetable per voice, and one glottal FIR, one set of converter tables
 * and (GVTM_PRECISION_F32) one noise-sample table for all of them.  n_voices == 1 makes exactly the plan gvtm_plan_create
 * makes.  GVTM_DEVICE_NONE works as for gvtm_plan_create.  A plan of two or more voices refuses the single-voice
 * entry points (gvtm_synthesize_batch_*, gvtm_stream_create, gvtm_synthesize_events_device) with
 * GVTM_ERR_INVALID_ARGUMENT; its event lists go through gvtm_synthesize_events_voices_device, with one track configuration
 * per voice (gvtm_plan_set_voice_tracks, "Parameter-track generation" below); gvtm_plan_info, gvtm_output_count and gvtm_output_capacity describe voice 0.  Its streams
 * come from gvtm_stream_create_voices ("Streams" below).  Reference model 5 has an entry of its own,
 * gvtm_plan_create_model5_voices. */
int    gvtm_plan_create_voices(const gvtm_config* configs, size_t n_voices, double control_rate, int device, gvtm_plan** plan_out);
/* The same for reference model 5: configs[n_voices], one gvtm5_config per voice (the 5_male voice's variants, say).
 * output_rate and precision (GVTM_PRECISION_F64) must be equal across configs (else GVTM_ERR_INVALID_ARGUMENT); every
 * other key may differ per voice, bypass and constant_radius_mouth_impedance included (none of them feeds a decision the
 * host makes for the launch).  A voice the design refuses, as gvtm_plan_create_model5 would, fails the call with a
 * message naming it ("voice 3: ...").  The device holds one constants block of each kind per voice and one set of
 * converter tables for all of them.  n_voices == 1 makes exactly the plan gvtm_plan_create_model5 makes; GVTM_DEVICE_NONE
 * gives a design-only plan; the rest is as for gvtm_plan_create_voices.  The kernel runs one utterance per workgroup
 * (the one-utterance shape of model 5), so voices whose internal rates differ (longer and shorter tracts) share a launch
 * without changing each other's shape. */
int    gvtm_plan_create_model5_voices(const gvtm5_config* configs, size_t n_voices, double control_rate, int device, gvtm_plan** plan_out);
/* The same for the float class, VocalTractModel5<float,1>: every config's precision must be GVTM_PRECISION_F32, and a voice
 * the float design refuses, as gvtm_plan_create_model5_float would, fails the call with a message naming it.  Voice v's
 * utterances come out bit for bit as a gvtm_plan_create_model5_float plan made from configs[v] synthesizes them.  One set
 * of float converter tables serves every voice.  The plan takes every several-voices entry point (synthesis, streams,
 * voice tracks and event lists); with n_voices == 1 it takes the single-voice entries as well.  The plan remembers that
 * this entry made it: a gvtm_plan_create_model5_float plan keeps refusing the gvtm_synthesize_voices_* entries.  The kernel
 * runs one utterance per workgroup in the float class's two shapes, chosen by the batch size as for one voice. */
int    gvtm_plan_create_model5_float_voices(const gvtm5_config* configs, size_t n_voices, double control_rate, int device, gvtm_plan** plan_out);
/* Number of voices of a plan (1 for gvtm_plan_create / _model5 / _model5_float plans); a negative status for a null plan. */
int    gvtm_plan_voice_count(const gvtm_plan* plan);
/* gvtm_plan_info of one voice (internal rate, control steps, converter increments and up-sampling differ by voice; model 5
 * voices: model5 = 1 and the voice's non-integer internal_rate_hz). */
int    gvtm_plan_voice_info(const gvtm_plan* plan, int voice, gvtm_info* info_out);
/* gvtm_output_count for an utterance of that voice; (size_t)-1 for a null plan or a voice out of range. */
size_t gvtm_voice_output_count(const gvtm_plan* plan, int voice, size_t n_frames);
/* max over voices of gvtm_output_capacity: the audio_stride for any mix of voices */
size_t gvtm_voices_output_capacity(const gvtm_plan* plan, size_t max_frames);

/* d_voice_ids [batch] int32: voice of each utterance, in any order; the rest as gvtm_synthesize_batch_device (NOTE the
 * order of max_frames and batch).  audio_stride >= gvtm_voice_output_count(plan, v, max_frames) for every voice v is
 * required, gvtm_voices_output_capacity(plan, max_frames) holds any mix.  An utterance whose voice id is outside
 * [0, n_voices) fails on its own, as a bad frame count does in the host entries: its out_counts = -1, maxabs = 0, its row
 * is left untouched; the call still succeeds.  Enqueue-only: a small grouping kernel sorts the utterances by voice on the
 * device (stable, each voice padded to whole workgroups), then one synthesis launch runs every voice.  The grouping's
 * scratch is the plan's: calls to this entry, to gvtm_synthesize_events_device and to gvtm_synthesize_events_voices_device
 * on one plan must be ordered on one stream (the host entries and streams have scratch of their own). */
int gvtm_synthesize_voices_device(gvtm_plan* plan, const float* d_params, const int32_t* d_frame_counts,
		const int32_t* d_voice_ids, size_t max_frames, size_t batch, float* d_audio, size_t audio_stride,
		int64_t* d_out_counts, float* d_maxabs, void* hip_stream);
/* Same with host buffers, through the three-stream pipeline of gvtm_synthesize_batch_host; a bad voice id or frame count
 * fails that utterance only (out_counts = -1, maxabs = 0, its row zeroed). */
int gvtm_synthesize_voices_host(gvtm_plan* plan, const float* params, const int32_t* frame_counts, const int32_t* voice_ids,
		size_t max_frames, size_t batch, float* audio, size_t audio_stride, int64_t* out_counts, float* maxabs);
/* As gvtm_synthesize_batch_host_pcm16 (scales = 0 for a failed utterance). */
int gvtm_synthesize_voices_host_pcm16(gvtm_plan* plan, const float* params, const int32_t* frame_counts, const int32_t* voice_ids,
		size_t max_frames, size_t batch, int16_t* pcm, size_t pcm_stride, int64_t* out_counts, float* maxabs, float* scales);

/* ---------------------------------------------------------------------------------------------
 * Ragged batches: packed in, packed out.
 *
 * Real batches are ragged (an utterance of 1 s next to one of 30 s).  The entries above take and return rectangles, so
 * the padding crosses PCIe and is staged on the device with everything else.  The packed entries take the utterances'
 * frames back to back and return their samples back to back, both described by offset tables, and what they stage on the
 * device is bounded by a slice of the batch, not by the batch.
 */
#define GVTM_PACKED_ALIGN 8   /* samples: every utterance starts at a multiple of it in the packed output */

/* Host-only, works on GVTM_DEVICE_NONE plans.  frame_offsets [batch+1] int64, non-decreasing from 0: utterance b owns
 * the frames [frame_offsets[b], frame_offsets[b+1]).  voice_ids [batch] or NULL (a one-voice plan; a plan of several voices
 * requires them).  Writes sample_offsets_out [batch+1] (may be NULL) and returns sample_offsets_out[batch], the
 * capacity (in samples) the output buffer needs; (size_t)-1 on a bad argument (the tables are checked as the synthesis
 * entries below check them).
 *   count[b]    = gvtm_voice_output_count(plan, voice b, frames b)      (exact, flush overrun included)
 *   offset[0]   = 0,  offset[b+1] = round_up(offset[b] + count[b], GVTM_PACKED_ALIGN) */
size_t gvtm_packed_sample_offsets(const gvtm_plan* plan, const int64_t* frame_offsets, const int32_t* voice_ids,
		size_t batch, int64_t* sample_offsets_out);

/* The packed form of gvtm_synthesize_voices_host (voice_ids given) resp. gvtm_synthesize_batch_host (voice_ids NULL, a
 * one-voice plan: the single-voice launch, so a gvtm_plan_create_model5_float plan takes NULL ids only).
 *   frames             [frame_offsets[batch]][16] float32: the utterances' frames back to back
 *   audio              [audio_capacity] float32, audio_capacity >= gvtm_packed_sample_offsets(...): utterance b's unscaled
 *                      samples occupy [offset[b], offset[b] + out_counts[b]); the gap up to offset[b+1] is written as
 *                      zeros, so the whole of [0, offset[batch]) is defined and nothing beyond it is touched
 *   sample_offsets_out [batch+1] the layout (may be NULL), out_counts [batch] (= the layout's counts), maxabs [batch]: may
 *                      be NULL
 * Samples, counts and peaks are bit for bit those the padded entry returns for the same utterance, in every precision,
 * for the models 0 to 4 and both classes of model 5, one voice or several.  An utterance of 0 frames is valid (the
 * converter's flush still yields samples).  Synchronous.
 *
 * All the tables are host memory, so a bad one refuses the whole call with GVTM_ERR_INVALID_ARGUMENT before any device
 * work: a null table or buffer where one is due; offsets that do not start at 0 or that decrease; a voice id outside
 * [0, n_voices) (the message names the first such utterance); NULL ids on a plan of several voices; an utterance whose
 * frames x control_steps does not fit the 31-bit step counter; a capacity below gvtm_packed_sample_offsets.  After these
 * a design-only plan returns GVTM_ERR_NO_DEVICE; batch == 0 returns GVTM_OK.
 *
 * Slices.  The utterances go in the caller's order, in contiguous slices, three staging sets deep on the plan's three
 * streams:   H2D packed frames(i+1) || unpack + synthesis + pack(i) || D2H packed output(i-1),   each D2H one contiguous
 * range [offset[lo], offset[hi]).  A slice of n utterances, the longest of F frames, holds in its set its packed frames,
 * its padded frames [n][F][16], its padded float samples [n][S] with S = gvtm_voices_output_capacity(plan, F) rounded up
 * to 8, and its packed output:
 *   set_bytes = 64 * n * F + 64 * frames_of_slice + 4 * n * S + w * aligned_samples_of_slice        (w = 4, int16: 2)
 * (aligned_samples_of_slice = offset[hi] - offset[lo]; the small per-utterance arrays -- offsets, counts, peaks, ids --
 * are the batch's and are not counted).  A slice is closed when the next utterance would exceed one machine-full
 * (utterances per compute unit x compute units) or, with a staging limit, when set_bytes would exceed limit / 3.  An
 * utterance that does not fit a set on its own refuses the call with GVTM_ERR_OUT_OF_MEMORY before any device work (the
 * message gives the bytes it needs).  The staging is the packed entries' own: they may not overlap each other on one
 * plan, the other entries are not affected.  Float plans: gvtm_plan_reserve runs once, for the longest utterance, before
 * the first slice. */
int gvtm_synthesize_packed_host(gvtm_plan* plan, const float* frames, const int64_t* frame_offsets, const int32_t* voice_ids,
		size_t batch, float* audio, size_t audio_capacity, int64_t* sample_offsets_out, int64_t* out_counts, float* maxabs);
/* The same ending as gvtm_synthesize_batch_host_pcm16 ends: int16 samples scaled by scales[b] = 0.95 / max|x[b]| (0 for
 * silence) and rounded, bit for bit the padded entry's; the gaps are zeros.  scales [batch] may be NULL. */
int gvtm_synthesize_packed_host_pcm16(gvtm_plan* plan, const float* frames, const int64_t* frame_offsets, const int32_t* voice_ids,
		size_t batch, int16_t* pcm, size_t pcm_capacity, int64_t* sample_offsets_out, int64_t* out_counts, float* maxabs,
		float* scales);

/* Upper bound, in bytes, on the three staging sets of the packed entries; 0 = none (the default).  Works on design-only
 * plans (it is kept).  Staging an earlier call left beyond the new limit is freed. */
int gvtm_plan_set_staging_limit(gvtm_plan* plan, size_t bytes);
/* staging_bytes: device bytes the three sets hold now (they stay allocated between calls and only grow; with a limit
 * never more than it); slices and largest_slice (utterances): of the last packed call that ran. */
typedef struct gvtm_packed_stats { size_t staging_bytes, limit, slices, largest_slice; } gvtm_packed_stats;
int gvtm_plan_packed_stats(const gvtm_plan* plan, gvtm_packed_stats* out);
/* Builds and uploads, synchronously, what the plan's launches of up to max_frames frames would otherwise build on first
 * use: the noise-sample table of a GVTM_PRECISION_F32 plan of the models 0 to 4.  GVTM_OK and nothing done for plans that
 * keep no table; GVTM_ERR_NO_DEVICE on a design-only plan.  Like the growth it replaces, it must not run while another
 * thread launches on the plan. */
int gvtm_plan_reserve(gvtm_plan* plan, size_t max_frames);

/* Page-locked host memory for the buffers of the host entries (hipHostMalloc, portable across devices), for callers
 * that do not link the HIP runtime themselves.  gvtm_host_free(NULL) is a no-op. */
int gvtm_host_alloc(size_t bytes, void** ptr_out);
void gvtm_host_free(void* ptr);

/* ---------------------------------------------------------------------------------------------
 * Streams: a batch of utterances synthesized piece by piece.
 *
 * The reference model is an object with state: every execSynthesisStep() continues where the last one stopped, and
 * the caller may read outputBuffer() whenever it likes (the editor does, after every step).  A gvtm_stream keeps that
 * state for `batch` independent utterances in device memory between launches: section delay lines, filter memories,
 * oscillator phase, noise seed, the decimator's and the converter's buffers and the converter's position.  Pushing an
 * utterance in any number of pieces and finishing it yields exactly the samples of the one-shot entry points
 * (bit for bit, in every precision).
 *
 *   gvtm_stream_push    appends frames; synthesizes every frame whose successor is known (the driver loop interpolates
 *                       each frame TOWARDS the next one, Controller.cpp:297-300), in multiples of a few frames (the
 *                       wavefronts' recurrences are unrolled: 12 internal steps), keeps the rest; returns the new samples
 *   gvtm_stream_finish  synthesizes what is kept (the last frame stands for its own successor, Controller.cpp:283) and
 *                       flushes the converter (finishSynthesis()); maxabs = max |sample| of the whole utterance
 *   gvtm_stream_reset   every utterance back to the state after construction (VocalTractModel::reset())
 *
 * Utterances pushed in lockstep (same frame counts every time) share workgroups like a one-shot batch; otherwise a
 * workgroup takes one utterance.  Plans of reference model 5 have streams too (vtm/VocalTractModel5.h:523-579: its scans,
 * filter memories, section flows, radiation-impedance memories, converter ring and the difference filter's look-back are
 * the state; pushes go in multiples of four internal steps).
 *
 * A plan of several voices has streams of gvtm_stream_create_voices: utterance b is spoken by voice voice_ids[b], and its
 * samples, counts and maxabs are, bit for bit and in every precision, those of a gvtm_stream_create stream on a
 * single-voice plan of that voice pushed with the same frames.  Each voice keeps its own granule of frames per push and
 * its own converter ring; lockstep is judged per voice (a workgroup only ever holds utterances of one voice), and model 5
 * runs one utterance per workgroup.  push, finish, reset and destroy take such a stream as they are; its capacity is the
 * largest over its voices.  Each launch first runs the grouping kernel of gvtm_synthesize_voices_device with the plan's
 * scratch: stream calls and gvtm_synthesize_voices_device calls on one plan must not overlap.
 *
 * A stream also takes its utterances as event lists, chunk by chunk, and generates their frames itself:
 * gvtm_stream_push_events, with gvtm_stream_get_drift / gvtm_stream_set_drift, declared behind the track-generation entries
 * below ("Streams fed event lists").  And as parameter targets, the interactive window's session: gvtm_stream_push_targets
 * and, for the one-voice plans of reference model 5, gvtm_stream_push_targets_model5; under the stream's several voices
 * gvtm_stream_push_targets_voices and gvtm_stream_push_targets_model5_voices ("Streams fed parameter targets").
 */
typedef struct gvtm_stream gvtm_stream;

int gvtm_stream_create(gvtm_plan* plan, size_t batch, gvtm_stream** stream_out);
/* A stream over a plan of one or more voices: utterance b is spoken by voice voice_ids[b] (host array of `batch`).
 * Refused with GVTM_ERR_INVALID_ARGUMENT for a null plan, stream_out or voice_ids or an empty batch, then for any id
 * outside [0, n_voices) (the message names the first such utterance; the ids are host memory, so the whole call is
 * refused), then with GVTM_ERR_NO_DEVICE for a design-only plan.  The state is sized for the plan's largest voice, so
 * that gvtm_stream_reset_voices never reallocates.  On a plan of one voice it is the stream gvtm_stream_create makes. */
int gvtm_stream_create_voices(gvtm_plan* plan, const int32_t* voice_ids, size_t batch, gvtm_stream** stream_out);
void gvtm_stream_destroy(gvtm_stream* stream);
/* (a stream of several voices keeps its voice ids) */
int gvtm_stream_reset(gvtm_stream* stream);
/* gvtm_stream_reset, then the utterances take new voices: voice_ids [batch] (host), checked as gvtm_stream_create_voices
 * checks them; a call refused for its arguments leaves the stream unchanged.  A device error after the checks leaves the
 * stream with the new ids, finished (pushes refused) until a reset succeeds.  A server reusing its utterance slots for
 * new clients. */
int gvtm_stream_reset_voices(gvtm_stream* stream, const int32_t* voice_ids);
/* Samples per utterance that a push of at most max_new_frames frames, or the finish after it, can return: the
 * audio_stride to allocate. */
size_t gvtm_stream_capacity(const gvtm_stream* stream, size_t max_new_frames);
/* params [batch][max_frames][16] float32 (host), frame_counts [batch] new frames per utterance or NULL (max_frames each);
 * audio [batch][audio_stride] float32 (host) receives the new samples of each utterance from index 0, out_counts[b]
 * how many (may be NULL); rows are zero beyond their count.  Synchronous. */
int gvtm_stream_push(gvtm_stream* stream, const float* params, const int32_t* frame_counts, size_t max_frames,
		float* audio, size_t audio_stride, int64_t* out_counts);
int gvtm_stream_finish(gvtm_stream* stream, float* audio, size_t audio_stride, int64_t* out_counts, float* maxabs);

/* Output scaling of Controller::writeOutputToBuffer / writeOutputToFile: scale = 0.95 / max|x|
 * (0 when max < 1e-30).  Exactly one of d_out_f32 / d_out_i16 may be non-NULL; i16 applies the
 * WAVEFileWriter rounding round(x * 32767). d_counts may be NULL (then audio_stride samples). */
int gvtm_normalize_batch_device(gvtm_plan* plan, const float* d_audio, size_t batch, size_t audio_stride,
		const int64_t* d_counts, const float* d_maxabs, float* d_out_f32, int16_t* d_out_i16,
		float* d_scales, void* hip_stream);

/* Average device time (ms) of the dominant synthesis kernel over the launches since the last
 * call, measured with HIP events on the launch stream; resets the accumulator.  Timing must
 * have been enabled with gvtm_plan_set_timing(plan, 1).  Returns < 0 when nothing was timed. */
int gvtm_plan_set_timing(gvtm_plan* plan, int enabled);
double gvtm_plan_take_kernel_ms(gvtm_plan* plan, int* launches_out);

/* ---------------------------------------------------------------------------------------------
 * Parameter-track generation: the step in front of the vocal-tract path, for a batch.
 * Replaces EventList::generateOutput() (vtm_control_model/EventList.cpp:930-1091) together with
 * DriftGenerator::drift() (vtm_control_model/DriftGenerator.cpp:72-84): event lists in, one
 * float32[16] frame per control period out, laid out as gvtm_synthesize_batch_device() reads them
 * (the frames never leave the device).  Bit-identical to the reference.
 */

/* One EventList event (vtm_control_model/EventList.h:117-160), flattened.  A parameter the event does
 * not set holds Event::EMPTY_PARAMETER = +infinity (HUGE_VAL). */
typedef struct gvtm_event {
	int32_t time_ms;     /* Event::time */
	int32_t has_interp;  /* Event::interpData present */
	double interp[4];    /* InterpolationData a, b, c, d (macro intonation, EventList.h:105-115) */
	double param[16];    /* Event::parameters */
	double special[16];  /* Event::specialParameters */
} gvtm_event;

typedef struct gvtm_track_config {
	int32_t control_period_ms;   /* EventList::controlPeriod_ (1..4), = 1000 / control rate */
	int32_t macro_intonation;    /* EventList flags (EventList.h:182-192) */
	int32_t micro_intonation;
	int32_t intonation_drift;
	int32_t smooth_intonation;
	int32_t reserved_;           /* must be 0 */
	double initial_pitch;        /* EventList::initialPitch_ (Controller.cpp:70) */
	double mean_pitch;           /* EventList::meanPitch_ = pitch_offset + reference_glottal_pitch (Controller.cpp:71) */
	double drift_deviation;      /* DriftGenerator::setUp(deviation, sampleRate, lowpassCutoff), Controller.cpp:73 */
	double drift_sample_rate;
	double drift_lowpass_cutoff;
} gvtm_track_config;

/* DriftGenerator state (noise seed, Butterworth filter memory).  The reference keeps one generator per
 * Controller, running on from chunk to chunk; a fresh one is {0.7892347, 0, 0, 0, 0}. */
typedef struct gvtm_drift_state {
	double seed, x1, x2, y1, y2;
} gvtm_drift_state;

/* Frames generateOutput() pushes for one event list (host-side, no device needed); (size_t)-1 on a
 * bad configuration. */
size_t gvtm_tracks_frame_count(const gvtm_track_config* config, const gvtm_event* events, size_t n_events);

/*
 * Batch generation, everything resident in device memory.
 *   d_events        all utterances' events back to back
 *   d_event_offsets [batch + 1] int64: utterance b owns events [offsets[b], offsets[b+1])
 *   d_params        [batch][max_frames][16] float32 out, 16-byte aligned (the frames leave as 16-byte stores;
 *                   GVTM_ERR_INVALID_ARGUMENT otherwise); frames beyond max_frames are dropped
 *   d_frame_counts  [batch] int32 out: frames generateOutput() produces (may exceed max_frames), may be NULL
 *   d_drift         [batch] in/out drift-generator states, or NULL: a fresh generator per utterance
 * d_params / d_frame_counts are exactly what gvtm_synthesize_batch_device() takes.
 */
int gvtm_generate_tracks_device(int device, const gvtm_track_config* config, const gvtm_event* d_events,
		const int64_t* d_event_offsets, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts,
		gvtm_drift_state* d_drift, void* hip_stream);

/*
 * Event lists in, audio out, in one call: gvtm_generate_tracks_device into a frame buffer the plan owns, then
 * gvtm_synthesize_batch_device, both enqueued on hip_stream (the frames never leave the device and the caller never sees
 * them).  Works for every plan, reference model 5 included.
 *   config          its control_period_ms must match the plan's control rate (1000 / control_rate)
 *   max_frames      frames per utterance the rows are sized for (gvtm_tracks_frame_count on the host); a list that yields
 *                   more is cut there
 *   d_frame_counts  [batch] int32 out: frames each list yields, may be NULL
 *   d_drift         [batch] in/out drift-generator states, or NULL (a fresh generator per utterance)
 * The remaining arguments are gvtm_synthesize_batch_device's.  The frame buffer is the plan's: calls to this entry, to
 * gvtm_synthesize_voices_device and to gvtm_synthesize_events_voices_device on one plan must be ordered on one stream (the
 * host entries and streams have buffers of their own).
 */
int gvtm_synthesize_events_device(gvtm_plan* plan, const gvtm_track_config* config, const gvtm_event* d_events,
		const int64_t* d_event_offsets, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream);

/*
 * Event lists of a batch that mixes voices.  Track generation depends on the voice: every reference Controller sets its
 * EventList's mean pitch to pitch_offset + reference_glottal_pitch of its voice variant (Controller.cpp:71; -12 / 0 / 2.5 /
 * 5 / 7.5 semitones for male / female / large_child / small_child / baby) and carries its own initial pitch, intonation
 * flags and drift generator set-up (Controller.cpp:70-81).  So a plan of several voices takes one gvtm_track_config per
 * voice, and the tracks kernel picks utterance b's by d_voice_ids[b].
 */

/* Per-voice track configurations of a plan: configs[n_configs], n_configs == gvtm_plan_voice_count(plan).  Synchronous:
 * designs each voice's drift filter and uploads the table into a buffer the plan owns.  Refused with
 * GVTM_ERR_INVALID_ARGUMENT, the message naming the voice ("voice 3: ..."): a null argument, n_configs different from the
 * plan's voice count, a configuration gvtm_tracks_frame_count would refuse, a control_period_ms that disagrees with the
 * plan's control rate.  Works on GVTM_DEVICE_NONE plans (the configurations are checked and kept on the host).  May be
 * called again; a refused call leaves the previous table in place.  It rewrites the table the queued kernels read: it must
 * not run while a gvtm_generate_tracks_voices_device / gvtm_synthesize_events_voices_device call on that plan is in flight. */
int gvtm_plan_set_voice_tracks(gvtm_plan* plan, const gvtm_track_config* configs, size_t n_configs);

/* gvtm_generate_tracks_device for a mix of voices: utterance b is generated under the plan's track configuration of voice
 * d_voice_ids[b] ([batch] int32, device memory) -- frames, frame counts and drift states bit for bit those of
 * gvtm_generate_tracks_device with that configuration.  The arguments follow gvtm_generate_tracks_device, with d_voice_ids
 * after the offsets (NOTE: batch before max_frames here, as in the events entries and unlike gvtm_synthesize_voices_*).
 * d_params must be 16-byte aligned.  Enqueue-only.  An utterance whose voice id is outside [0, n_voices) fails on its
 * own: d_frame_counts[b] = 0, its row of d_params and d_drift[b] are left untouched; the call still succeeds.
 * GVTM_ERR_INVALID_ARGUMENT before gvtm_plan_set_voice_tracks has succeeded on the plan, GVTM_ERR_NO_DEVICE on a design-only
 * plan; batch == 0 returns GVTM_OK.  Takes a one-voice plan too, and plans of reference model 5 (the frames do not depend
 * on the vocal-tract model). */
int gvtm_generate_tracks_voices_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_event_offsets,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts,
		gvtm_drift_state* d_drift, void* hip_stream);

/* gvtm_synthesize_events_device for a mix of voices: gvtm_generate_tracks_voices_device into the plan's frame buffer, then
 * gvtm_synthesize_voices_device, both enqueued on hip_stream.  The arguments follow gvtm_synthesize_events_device, with
 * d_voice_ids after the offsets (NOTE: batch before max_frames, unlike gvtm_synthesize_voices_*) and the track
 * configurations taken from the plan.  Voice v's utterances come out bit for bit -- samples, counts, peaks, frame counts,
 * drift states -- as gvtm_synthesize_events_device on a single-voice plan of that voice with that voice's configuration.
 * audio_stride is checked per voice as in gvtm_synthesize_voices_device.  An utterance whose voice id is outside
 * [0, n_voices) fails on its own: frame_counts = 0, out_counts = -1, maxabs = 0, its audio row and drift state are left
 * untouched; the call still succeeds.  Status codes and the one-voice and model-5 plans as for
 * gvtm_generate_tracks_voices_device.  The frame buffer and the grouping's scratch are the plan's: calls to this entry, to
 * gvtm_synthesize_events_device and to gvtm_synthesize_voices_device on one plan must be ordered on one stream (the host
 * entries and streams have buffers of their own and may overlap with it). */
int gvtm_synthesize_events_voices_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_event_offsets,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream);

/*
 * Utterances of several event lists.  The reference builds an utterance that way: Controller::getParametersFromPhoneticString
 * (Controller.cpp:141-154) cuts the phonetic string at its /c markers (the text parser emits one chunk per phrase) and, per
 * chunk, runs eventList_.setUp(), parses and calls eventList_.generateOutput(vtmParamList_) on the same parameter list: the
 * utterance's frames are the chunks' frames one after the other, and the drift generator (one per Controller, never
 * reseeded) runs on from chunk to chunk.  Here two offset tables describe the batch:
 *   chunk_offsets  [n_chunks + 1] int64, non-decreasing: chunk c owns the events [chunk_offsets[c], chunk_offsets[c+1])
 *   utt_chunks     [batch + 1] int64, non-decreasing: utterance b owns the chunks [utt_chunks[b], utt_chunks[b+1])
 * Each chunk is generated as a list of its own (values, deltas, intonation polynomial and time start again, as in a fresh
 * generateOutput() call); a chunk of fewer than two events yields nothing and leaves the drift state alone, an utterance
 * without chunks yields 0 frames.
 */

/* Frames of one utterance of n_chunks chunks: the sum over the chunks of gvtm_tracks_frame_count (host-side, no device
 * needed).  (size_t)-1 on a bad configuration, on a null argument with n_chunks > 0 (a null config always) and on offsets
 * that decrease; 0 for n_chunks == 0. */
size_t gvtm_tracks_chunks_frame_count(const gvtm_track_config* config, const gvtm_event* events,
		const int64_t* chunk_offsets, size_t n_chunks);

/* gvtm_generate_tracks_voices_device for utterances of several chunks, in one launch for the whole batch (the tables are
 * device memory: the host never learns a count).  The frames of utterance b are the concatenation, over its chunks, of the
 * frames gvtm_generate_tracks_voices_device yields for the chunk as a list of its own under voice d_voice_ids[b], the drift
 * state a chunk leaves being the next chunk's; d_drift[b] leaves as the last chunk left it.  d_frame_counts[b] is the
 * utterance's total, and max_frames is per utterance, all chunks together: frames beyond it are dropped, the count and the
 * drift state still cover all of them.  With one chunk per utterance everything is bit for bit the voices entry's.
 * Everything not named here -- the track configurations (gvtm_plan_set_voice_tracks), the order of the checks and the
 * status codes, the 16-byte alignment of d_params, batch == 0, a voice id outside [0, n_voices), enqueue-only, one-voice
 * and model-5 plans -- is gvtm_generate_tracks_voices_device's; a null d_utt_chunks is refused with the other nulls. */
int gvtm_generate_tracks_chunks_device(gvtm_plan* plan, const gvtm_event* d_events,
		const int64_t* d_chunk_offsets,   /* [n_chunks + 1] event offsets, non-decreasing */
		const int64_t* d_utt_chunks,      /* [batch + 1]: utterance b owns chunks [d_utt_chunks[b], d_utt_chunks[b+1]) */
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_params,
		int32_t* d_frame_counts, gvtm_drift_state* d_drift, void* hip_stream);

/* gvtm_synthesize_events_voices_device for utterances of several chunks: gvtm_generate_tracks_chunks_device into the
 * plan's frame buffer, then gvtm_synthesize_voices_device on its frames and counts, both enqueued on hip_stream -- one
 * track per utterance, as the reference synthesizes the whole parameter list at once (one vocal-tract state, one
 * converter flush, one peak).  Samples, counts, peaks, frame counts and drift states are bit for bit those of the two
 * calls made separately.  Checks, status codes, a bad voice id, the plans accepted and the one-stream ordering rule of the
 * plan's frame buffer and grouping scratch as for gvtm_synthesize_events_voices_device. */
int gvtm_synthesize_events_chunks_device(gvtm_plan* plan, const gvtm_event* d_events,
		const int64_t* d_chunk_offsets, const int64_t* d_utt_chunks, const int32_t* d_voice_ids,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts,
		int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream);

/*
 * Intonation contours applied to event lists.  Controller::synthesizeFromEventListToBuffer/File (Controller.cpp:158-168,
 * 210-224) keeps the event list and changes the intonation: clearMacroIntonation(), prepareMacroIntonationInterpolation()
 * (EventList.cpp:822-900, 1093-1099) from the list of IntonationPoints, then generateOutput() -- the editor's path after
 * every edit of the contour, and for a batch one sentence spoken under many contours.  The entries below make the list
 * those two calls leave, on the host or for a batch on the device, where many utterances may share one base list and
 * only the points (24 bytes each) differ between them.
 *
 * The rule, for a base list of E events and P points under a configuration's control_period_ms (cp) and
 * smooth_intonation:
 *   1. every base event is kept bit for bit, except has_interp = 0 and interp = {0, 0, 0, 0} (also with P = 0);
 *   2. duration = time of the last base event + 100, taken once, before anything is inserted (setFullTimeScale, :679-684);
 *   3. point j: t = time_ms < 0 ? 0 : time_ms; q_j = (int)t, and with cp != 1, q_j -= q_j % cp (insertEvent, :302-315);
 *   4. the merged list is the base list plus one event per q_j that no base event has, in the order of their times; a new
 *      event has all 32 parameters at +infinity, has_interp = 0 and interp = 0;
 *   5. with P >= 2 the event at q_j (j < P - 1) gets has_interp = 1 and the polynomial of :844-883 from x1 = q_j,
 *      x2 = q_{j+1} (the events' times, not the points'), y = semitone, m = slope -- the cubic a, b, c, d in the reference's
 *      order of operations with coef = 1.0 / (dx * dx * dx), or, linear, a = (y2 - y1) / dx, b = y1 - x1 * a, c = d = 0 --
 *      and the event at q_{P-1} gets {0, 0, 0, semitone} (smooth) or {0, semitone, 0, 0} (linear);
 *   6. with P = 1 the event at q_0 exists and no event carries a polynomial (the reference's loop does not run).
 * Double arithmetic without FMA contraction on the host and on the device: bit for bit the reference's list.
 *
 * An utterance is refused on its own: its merged list has 0 events, so track generation gives it 0 frames and leaves its
 * drift state alone.  Its status says why; the first that applies, every point being looked at for 3 before any for 4:
 *   0  ok
 *   1  empty base list; on the device also a list id outside [0, n_lists) or a voice id outside the plan's voices, on the
 *      host also base times that are negative or not strictly increasing (the device does not look)
 *   2  more than GVTM_MAX_INTONATION_POINTS points (on the device also point offsets that decrease)
 *   3  a time_ms that is not finite or greater than duration + cp: insertEvent returns null and the reference throws
 *      (:307-309, :829-842); also a time of 2^31 ms or more, which a list that ends within 100 ms of INT_MAX would admit
 *   4  q_j not strictly increasing: the reference would compute 1 / 0 (its own addIntonationPoint keeps points two control
 *      periods apart, :915-924); refused on purpose rather than restated
 *   5  device only: the merged list does not fit behind the lists before it in out_capacity events
 */
typedef struct gvtm_intonation_point {
	double time_ms;   /* IntonationPoint::absoluteTime(): beat of its rule + offset, IntonationPoint.cpp:43-52 */
	double semitone;  /* IntonationPoint::semitone() */
	double slope;     /* IntonationPoint::slope() (used with smooth_intonation only) */
} gvtm_intonation_point;
#define GVTM_MAX_INTONATION_POINTS 64   /* per utterance */

/* The rule on the host; needs no device.  Returns the merged events (>= 0; 0 with *status_out != 0 for a refused
 * utterance), or -1 on a bad call: a null config or status_out, a config gvtm_tracks_frame_count would refuse, null
 * events / points with a count > 0, a capacity too small for the merged list.  events_out == NULL: count and status only
 * (capacity is not read).  The merged list holds at most n_events + n_points events.  gvtm_tracks_frame_count on the merged
 * list gives the frames generateOutput() yields for it: what to size max_frames with below.  (A bound without the walk:
 * the last merged event lies at duration + cp at most, duration the last base event's time + 100, so no more than
 * ceil((last base time + 100 + cp) / cp) + n_events + n_points frames.) */
int64_t gvtm_intonation_apply_host(const gvtm_track_config* config, const gvtm_event* events, size_t n_events,
		const gvtm_intonation_point* points, size_t n_points, gvtm_event* events_out, size_t capacity, int32_t* status_out);

/* The rule for a batch, everything resident in device memory.
 *   d_events, d_list_offsets [n_lists + 1]   base list l owns the events [off[l], off[l+1])
 *   d_list_ids [batch] int32, or NULL        utterance b's base list; NULL: n_lists == batch and utterance b uses list b.
 *                                            Many utterances may share one base list.
 *   d_points, d_point_offsets [batch + 1]    utterance b owns the points [off[b], off[b+1])
 *   d_voice_ids [batch] int32                as the chunks entry takes them: smooth_intonation comes from the plan's track
 *                                            configuration of the utterance's voice (gvtm_plan_set_voice_tracks), the
 *                                            control period is the plan's
 *   d_events_out                             out, out_capacity events: the merged lists back to back.  The caller sizes it
 *                                            as the sum over b of E(list of b) + P_b, which it knows from its host tables
 *   d_event_offsets_out [batch + 1]          out: exactly the d_event_offsets the tracks entries take
 *   d_status [batch] int32, may be NULL      out: the statuses above
 * Merged lists, offsets and statuses are bit for bit gvtm_intonation_apply_host's, utterance by utterance.  Nothing is
 * written at or beyond out_capacity events and nothing for a refused utterance; a list that would end beyond out_capacity
 * is refused (5) and takes no room, so a shorter one behind it may still fit.  Enqueue-only: three small kernels on
 * hip_stream, no scratch.  Refused before any device work, in this order: a null plan, a plan without track
 * configurations, with batch > 0 a null argument (d_list_ids and d_status aside) or a NULL d_list_ids with n_lists !=
 * batch (GVTM_ERR_INVALID_ARGUMENT); a design-only plan (GVTM_ERR_NO_DEVICE); batch == 0 returns GVTM_OK. */
int gvtm_apply_intonation_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_list_offsets, size_t n_lists,
		const int32_t* d_list_ids, const gvtm_intonation_point* d_points, const int64_t* d_point_offsets,
		const int32_t* d_voice_ids, size_t batch, gvtm_event* d_events_out, size_t out_capacity,
		int64_t* d_event_offsets_out, int32_t* d_status, void* hip_stream);

/* The three steps behind one call: gvtm_apply_intonation_device into an event buffer the plan owns (grown to
 * events_capacity events: the out_capacity above), then gvtm_synthesize_events_voices_device on the merged lists, all
 * enqueued on hip_stream.  Samples, counts, peaks, frame counts, drift states and statuses are bit for bit those of the
 * calls made separately; a refused utterance has 0 frames.  max_frames: gvtm_tracks_frame_count on the host-applied list,
 * or the bound given with gvtm_intonation_apply_host.  The remaining arguments, checks, status codes and the one-stream
 * ordering rule are gvtm_synthesize_events_voices_device's (the event buffer is one more of the plan's that the rule
 * covers); the apply entry's refusals come first, then a null audio buffer and the stride. */
int gvtm_synthesize_intonation_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_list_offsets,
		size_t n_lists, const int32_t* d_list_ids, const gvtm_intonation_point* d_points, const int64_t* d_point_offsets,
		const int32_t* d_voice_ids, size_t events_capacity, size_t batch, size_t max_frames, float* d_audio,
		size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift,
		int32_t* d_status, void* hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter-modification gestures applied to frames.  The editor's parameter-modification window keeps an utterance's
 * parameter list and, while the utterance plays, lets the user drag one of the 16 parameters; its processor smooths the
 * drag with a 20 ms MovingAverageFilter<float> at the internal rate and writes original + filtered or original * filtered
 * into every control frame (gama_tts_editor ParameterModificationSynthesis.cpp:117-194); "synthesize to file" hands the
 * modified list to Controller::synthesizeToFile (ParameterModificationWindow.cpp:200-231, 281-322).  The entries below make
 * the modified list, on the host or for a batch on the device, where many utterances may share one base list of frames and
 * only the gestures' points (8 bytes each) differ between them.
 *
 * The rule, for base frames orig[F][16] (float), the voice's control_steps (cs) and N = (size_t)roundf((float)
 * internal_rate_hz * (float)20.0e-3) -- a float product rounded half away from zero; gvtm_modification_filter_length gives
 * it -- with invN = 1.0 / N in double.  An utterance has G gestures, applied in order; a gesture is a parameter p, an
 * operation (GVTM_MODIFICATION_ADD or GVTM_MODIFICATION_MULTIPLY) and points (step_j, value_j): internal steps from the
 * start of playback, strictly increasing, and float values.  The processor reads at most one modification per internal
 * step, so every such list is something the reference can be made to do.
 *   out = orig
 *   for each gesture, in order (a fresh run: prepareSynthesis() resets the filter):
 *     cur = none
 *     for k = 1 .. F-1 (frame 0 is never modified), for i = 0 .. cs-1:
 *       s = (k-1)*cs + i;  if the next point has step == s: cur = its value
 *       if cur != none:
 *         at the first filter call ever: ring[0 .. N) = cur; sum = (double)cur * (double)N
 *         sum = sum - (double)ring[pos]; sum = sum + (double)cur; ring[pos] = cur; pos advances
 *         fm = (float)(sum * invN)
 *         if i == 0: out[k][p] = ADD ? orig[k][p] + fm : orig[k][p] * fm      (float arithmetic)
 * What follows from it:
 *   - points at or beyond step (F-1)*cs never act, and a gesture without an acting point changes nothing;
 *   - a gesture reads orig, never out: on one parameter a later gesture overwrites an earlier one from its own first frame
 *     ceil(step_0 / cs) + 1 to the end and leaves the frames before alone; gestures on different parameters accumulate;
 *   - the two additions into sum are sequential double operations, each rounded, in this order: with values spread over
 *     many decades the result differs from the exactly rounded window mean, and it is the sequential one that is computed,
 *     without FMA contraction on the host and on the device: bit for bit the reference's frames (an orig entry that is NaN
 *     gives a NaN whose sign and payload may differ: the NaN exception of the synthesis entries).
 *
 * An utterance is refused on its own: no frame of its output is written, and on the device its frame count is 0.  Its
 * status says why; the first that applies, every gesture and point being looked at for 3 before any for 4:
 *   0  ok
 *   1  a base of fewer than 2 frames (the window's validData()); on the device also a base id outside [0, n_bases), a voice
 *      id outside the plan's voices, a base of more than max_frames frames
 *   2  more than GVTM_MAX_GESTURES gestures (on the device also gesture or point offsets that decrease or are negative)
 *   3  a parameter outside [0, 16), an operation other than 0 / 1, a point value that is not finite
 *   4  a negative step; steps not strictly increasing within a gesture
 */
#define GVTM_MODIFICATION_ADD 0
#define GVTM_MODIFICATION_MULTIPLY 1
#define GVTM_MAX_GESTURES 64   /* per utterance */

/* N of the rule for a voice of the plan; -1 on a null plan or a voice outside the plan's.  Host only: works on
 * GVTM_DEVICE_NONE plans. */
int64_t gvtm_modification_filter_length(const gvtm_plan* plan, int voice);

/* The rule on the host for one utterance under voice `voice` of the plan (its control_steps and N); needs no device and
 * works on GVTM_DEVICE_NONE plans.
 *   frames [n_frames][16]                        the base frames
 *   gestures [n_gestures][2] int32               (parameter, operation) of gesture g
 *   gesture_offsets [n_gestures + 1]             gesture g owns the points [off[g], off[g+1])
 *   point_steps int32, point_values float        the points of all gestures back to back
 *   frames_out [n_frames][16]                    out: the modified frames; must not overlap frames
 *   status_out                                   out: the status above; a refused utterance leaves frames_out untouched
 * GVTM_ERR_INVALID_ARGUMENT for a null plan, status_out or frames_out, null frames with n_frames > 0, null tables with
 * counts > 0, a voice outside the plan's, gesture_offsets that are negative or decrease. */
int gvtm_modification_apply_host(const gvtm_plan* plan, int voice, const float* frames, size_t n_frames,
		const int32_t* gestures, const int64_t* gesture_offsets, size_t n_gestures, const int32_t* point_steps,
		const float* point_values, float* frames_out, int32_t* status_out);

/* The rule for a batch, everything resident in device memory.
 *   d_base_params [n_bases][max_frames][16], d_base_frame_counts [n_bases] int32
 *                                            base l holds d_base_frame_counts[l] frames at the start of its row
 *   d_base_ids [batch] int32, or NULL        utterance b's base; NULL: n_bases == batch and utterance b uses base b.  Many
 *                                            utterances may share one base.
 *   d_gestures [n][2] int32, d_gesture_offsets [n + 1], d_utt_gestures [batch + 1]
 *                                            the two-level tables of the chunks entries: utterance b owns the gestures
 *                                            [d_utt_gestures[b], d_utt_gestures[b+1]), gesture g (parameter, operation) =
 *                                            d_gestures[g] and the points [d_gesture_offsets[g], d_gesture_offsets[g+1])
 *   d_point_steps int32, d_point_values float
 *   d_voice_ids [batch] int32, or NULL       utterance b's voice (its control_steps and N); NULL on a one-voice plan
 *   d_params_out [batch][max_frames][16]     out: utterance b's row holds the modified frames in its first F frames,
 *                                            [F, max_frames) of the row is untouched; a refused utterance's row is untouched
 *   d_frame_counts_out [batch] int32         out: F, or 0 for a refused utterance
 *   d_status [batch] int32, may be NULL      out: the statuses above
 * d_params_out and d_frame_counts_out are exactly what gvtm_synthesize_voices_device and gvtm_synthesize_batch_device take.
 * Frames, counts and statuses are bit for bit gvtm_modification_apply_host's, utterance by utterance.  d_base_params and
 * d_params_out must be 16-byte aligned and must not overlap (not checked).  Works on every plan.  Enqueue-only: two small
 * kernels on hip_stream, no scratch.  Refused before any device work, in this order: a null plan; with batch > 0 a null
 * table, buffer or count array (d_base_ids, d_status and, on a one-voice plan, d_voice_ids aside), a NULL d_base_ids with
 * n_bases != batch, a NULL d_voice_ids on a plan of several voices, a misaligned buffer (GVTM_ERR_INVALID_ARGUMENT); a
 * design-only plan (GVTM_ERR_NO_DEVICE), with batch == 0 too, as the neighbouring entries: without a device there is no
 * call; on a plan with a device batch == 0 returns GVTM_OK and nothing but the plan is looked at. */
int gvtm_apply_modifications_device(gvtm_plan* plan, const float* d_base_params, const int32_t* d_base_frame_counts,
		size_t n_bases, const int32_t* d_base_ids, const int32_t* d_gestures, const int64_t* d_gesture_offsets,
		const int64_t* d_utt_gestures, const int32_t* d_point_steps, const float* d_point_values,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_params_out, int32_t* d_frame_counts_out,
		int32_t* d_status, void* hip_stream);

/* The two steps behind one call: gvtm_apply_modifications_device into the plan's frame buffer (the one the events entries
 * use), then the synthesis launch on it with the plan's grouping scratch -- gvtm_synthesize_voices_device with
 * d_voice_ids, gvtm_synthesize_batch_device with NULL ids (a gvtm_plan_create_model5_float plan takes NULL ids only) -- all
 * enqueued on hip_stream.  Samples, counts, peaks, frame counts and statuses are bit for bit those of the two calls made
 * separately; a refused utterance is synthesized as one of 0 frames.  d_frame_counts [batch] int32 may be NULL.  The
 * remaining arguments, checks and the one-stream ordering rule are gvtm_synthesize_events_voices_device's; the apply
 * entry's refusals come first, then a null audio buffer and the stride, then a design-only plan. */
int gvtm_synthesize_modified_device(gvtm_plan* plan, const float* d_base_params, const int32_t* d_base_frame_counts,
		size_t n_bases, const int32_t* d_base_ids, const int32_t* d_gestures, const int64_t* d_gesture_offsets,
		const int64_t* d_utt_gestures, const int32_t* d_point_steps, const float* d_point_values,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Synthesis from parameter targets.  The editor's interactive window drives the model without control frames: the user sets
 * targets for the 16 parameters, and on every internal step each parameter passes through its own MovingAverageFilter<float>
 * of 50 ms into setParameter() before execSynthesisStep() runs (gama_tts_editor/src/interactive/InteractiveAudio.cpp:
 * 164-186).  There is no linear interpolation: the parameters move on every internal sample.  The entries below do that for a
 * batch: an utterance is a step count and, per parameter, a handful of (step, value) points, and the filter runs inside the
 * synthesis kernel, so nothing but the points (8 bytes each) is read per utterance.
 *
 * The rule, for a voice with internal rate r: N = (size_t)roundf((float)r * (float)50.0e-3) -- a float product rounded half
 * away from zero (at 20 050 Hz the product is 1002.5 and N is 1003); gvtm_targets_filter_length gives it -- and invN =
 * 1.0 / N in double.  An utterance is S internal steps and per parameter p a list of points (step_j, value_j): int32 steps
 * that strictly increase, float values.
 *   cur[p] = 0.0f for every p                      (paramValues_ starts at 0, InteractiveAudio.cpp:106-108)
 *   for s = 0 .. S-1:
 *     for p = 0 .. 15:
 *       if list p's next point has step == s: cur[p] = its value
 *       at s == 0: ring_p[0 .. N) = cur[p]; sum_p = (double)cur[p] * (double)N      (the filter's first call)
 *       sum_p = sum_p - (double)ring_p[pos]; sum_p = sum_p + (double)cur[p]; ring_p[pos] = cur[p]; pos advances
 *       v[s][p] = (float)(sum_p * invN);  setParameter(p, v[s][p])
 *     execSynthesisStep()
 *   finishSynthesis()
 * What follows from it:
 *   - points at or beyond step S never act;
 *   - a parameter without a point at step 0 is held at 0 until its first point (and a list without points at 0 throughout);
 *   - the two additions into sum are sequential double operations, each rounded, in this order, without FMA contraction on
 *     the host and on the device; (double)cur * N is rounded before cur is taken from it.  With values spread over many
 *     decades the result differs from the exactly rounded window mean, and it is the sequential one that is computed;
 *   - the window itself reads its parameter ring buffer only between bursts of steps, so its sessions are the lists whose
 *     steps fall on those boundaries; the rule lets a target act at any step;
 *   - the window never calls finishSynthesis(); the one-shot entry does, as every gvtm_synthesize_batch_* entry does;
 *   - the samples are, by definition, what gvtm_synthesize_batch_device returns for the same voice on a plan whose control
 *     rate is its internal rate (control_steps == 1) fed v[s][0 .. 16) as frame s: that route runs S frames as S steps, and
 *     frame s is used unchanged at step s (Controller.cpp:294-311).
 *
 * An utterance is refused on its own and synthesized as one of 0 steps (exactly as a frame count of 0 is).  Its status says
 * why; the first that applies, every point being looked at for 3 before any for 4:
 *   0  ok
 *   1  a step count that is negative, above max_steps (host: beyond the kernels' 31-bit step counter); a list id outside
 *      [0, n_lists)
 *   2  list offsets that are negative or decrease
 *   3  a value that is not finite
 *   4  a negative step; steps not strictly increasing within a list
 *   5  gvtm_synthesize_targets_voices_device and gvtm_synthesize_targets_model5_voices_device only: a voice id outside [0, n_voices).  Looked at before every other status;
 *      such an utterance is not one of 0 steps but left out as gvtm_synthesize_voices_device leaves it out: out_counts -1,
 *      maxabs 0, its audio row untouched
 */

/* N of the rule for a voice of the plan; -1 on a null plan or a voice outside the plan's.  Host only: works on
 * GVTM_DEVICE_NONE plans. */
int64_t gvtm_targets_filter_length(const gvtm_plan* plan, int voice);

/* The samples finishSynthesis() leaves after n_steps internal steps of the plan's (first) voice, flush overrun included, and
 * the row length that holds every utterance of up to max_steps steps (larger on down-sampling plans, as
 * gvtm_output_capacity is): gvtm_output_count and gvtm_output_capacity by steps, independent of the plan's control rate.
 * (size_t)-1 on a null plan. */
size_t gvtm_targets_output_count(const gvtm_plan* plan, size_t n_steps);
size_t gvtm_targets_output_capacity(const gvtm_plan* plan, size_t max_steps);

/* The rule's v[s][p] on the host for one utterance under voice `voice` of the plan (its N); needs no device and works on
 * GVTM_DEVICE_NONE plans.
 *   list_offsets [17]                            parameter p owns the points [off[p], off[p+1])
 *   point_steps int32, point_values float        the points of all lists back to back
 *   frames_out [n_steps][16]                     out: v; a refused utterance leaves it untouched
 *   status_out                                   out: the status above
 * GVTM_ERR_INVALID_ARGUMENT for a null plan, status_out or list_offsets, null frames_out with n_steps > 0, null point tables
 * with points, a voice outside the plan's. */
int gvtm_targets_apply_host(const gvtm_plan* plan, int voice, const int64_t* list_offsets, const int32_t* point_steps,
		const float* point_values, int64_t n_steps, float* frames_out, int32_t* status_out);

/* The rule from any step: v[first_step .. first_step + n_steps) of the same utterance, given the 16 sums as they stood after
 * step first_step - 1.  The points keep their absolute steps.  In front of a step s0 > 0 parameter p stands as follows:
 *   cur[p]       the value of its last point with step <= s0 - 1, or 0.0f without one
 *   the value that leaves the window at step s (s >= s0): the one fed at step s - N, which is the value of the last point
 *                with step <= s - N; for s < N, and where no point is that early, the value fed at step 0 (the point at
 *                step 0, or 0.0f)
 *   sum_p        carried: the double additions of floats many decades apart are not exact, so the sum cannot be formed
 *                again from the points
 * So a list may forget: in front of step s0 a point is no longer needed once its successor has step <= s0 - 1 - N; what is
 * kept is the last point at or before the window's far edge s0 - 1 - N and every later one.  A list trimmed that way gives
 * the same bytes.
 *   first_step == 0          gvtm_targets_apply_host: the sums are not read
 *   sums_inout [16] double   in (first_step > 0): the sums after step first_step - 1; out: the sums after the last step
 *   frames_out [n_steps][16] out: frames_out[0] is step first_step's
 * The same checks, the same statuses; a negative first_step is status 1, and so is a first_step + n_steps beyond the kernels'
 * step counter.  GVTM_ERR_INVALID_ARGUMENT as gvtm_targets_apply_host, and for a null sums_inout. */
int gvtm_targets_apply_host_from(const gvtm_plan* plan, int voice, const int64_t* list_offsets, const int32_t* point_steps,
		const float* point_values, int64_t first_step, int64_t n_steps, double* sums_inout, float* frames_out,
		int32_t* status_out);

/* The rule and the synthesis for a batch in one launch, everything resident in device memory.
 *   d_list_offsets [n_lists + 1]                 list l owns the points [off[l], off[l+1]) of d_point_steps / d_point_values
 *   d_list_ids [batch][16] int32, or NULL        the list of utterance b's parameter p; NULL: n_lists == 16 * batch and it is
 *                                                list 16 b + p.  Many utterances may share a list: a study that moves one
 *                                                articulator shares the other fifteen.
 *   d_step_counts [batch] int32, or NULL         utterance b's steps S; NULL: all max_steps
 *   d_audio [batch][audio_stride], d_out_counts [batch] (may be NULL), d_maxabs [batch] (may be NULL)
 *                                                as gvtm_synthesize_batch_device's; utterance b yields
 *                                                gvtm_targets_output_count(plan, S_b) samples
 *   d_status [batch] int32, may be NULL          out: the statuses above
 * Samples, counts and peaks are those of gvtm_synthesize_batch_device on gvtm_targets_apply_host's frames at one step per
 * frame (above), in float bit for bit.  One-voice plans of the models 0 to 4, every precision.  Enqueue-only -- a small check
 * kernel (one wavefront per utterance: statuses and step counts into the plan's scratch) and the synthesis launch on
 * hip_stream -- with the batch entry's one exception: a float plan's noise table grows to max_steps steps
 * (gvtm_plan_reserve(plan, frames) reserves frames * control_steps of them).  Calls on one plan must be ordered on one stream,
 * as the events entries'.  Refused before any device work, in this order: a null plan; with batch > 0 a null offset table,
 * point table or audio buffer, a NULL d_list_ids with n_lists != 16 * batch, a max_steps beyond the step counter, a stride
 * below gvtm_targets_output_capacity(plan, max_steps) (GVTM_ERR_INVALID_ARGUMENT); a plan of several voices or a model 5
 * plan (GVTM_ERR_UNSUPPORTED); a design-only plan (GVTM_ERR_NO_DEVICE), with batch == 0 too; on a plan with a device
 * batch == 0 returns GVTM_OK.  A plan of several voices has gvtm_synthesize_targets_voices_device (below). */
int gvtm_synthesize_targets_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts, size_t batch,
		size_t max_steps, float* d_audio, size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status,
		void* hip_stream);

/* gvtm_targets_output_count for voice `voice` of a plan of several voices, and the row length that holds every utterance of
 * up to max_steps steps under any voice of the plan: the largest of the voices' gvtm_targets_output_capacity.  What
 * gvtm_voice_output_count and gvtm_voices_output_capacity are to the frame entries, by steps.  Host only: they work on
 * GVTM_DEVICE_NONE plans.  (size_t)-1 on a null plan, the count also for a voice outside the plan's. */
size_t gvtm_targets_voice_output_count(const gvtm_plan* plan, int voice, size_t n_steps);
size_t gvtm_targets_voices_output_capacity(const gvtm_plan* plan, size_t max_steps);

/* gvtm_synthesize_targets_device with a voice id per utterance: one articulator trajectory under every speaker in one launch.
 *   d_voice_ids [batch] int32                    utterance b walks its lists under voice d_voice_ids[b] of the plan: that
 *                                                voice's own N = gvtm_targets_filter_length(plan, voice) and 1 / N.  Lists
 *                                                hold no N, so utterances of different voices may share a list
 *   d_audio [batch][audio_stride]                utterance b yields gvtm_targets_voice_output_count(plan, voice_b, S_b) samples
 *   every other argument                         as gvtm_synthesize_targets_device's
 * In every precision voice v's utterances come out bit for bit -- samples, out_counts, maxabs -- as
 * gvtm_synthesize_targets_device synthesizes them on a one-voice plan made from configs[v].  A voice id outside
 * [0, n_voices) is status 5 (above); an utterance refused with status 1 to 4 is one of 0 steps of its voice.  Plans of the
 * models 0 to 4 of any number of voices: on a plan of one voice (gvtm_plan_create, or gvtm_plan_create_voices with one
 * config) ids that are all 0 give gvtm_synthesize_targets_device's bytes.  Enqueue-only -- the check kernel, the grouping
 * kernel of gvtm_synthesize_voices_device and the synthesis launch on hip_stream -- with the same exception: a float plan's
 * noise table grows to max_steps steps.  The call uses the plan's grouping scratch and step-count scratch: calls on one plan
 * must be ordered on one stream, as gvtm_synthesize_voices_device's.  Refused before any device work, in this order: a null
 * plan; with batch > 0 what gvtm_synthesize_targets_device refuses, NULL d_voice_ids, a stride below
 * gvtm_targets_voices_output_capacity(plan, max_steps) (GVTM_ERR_INVALID_ARGUMENT); a model 5 plan of either class
 * (GVTM_ERR_UNSUPPORTED); a design-only plan (GVTM_ERR_NO_DEVICE), with batch == 0 too; on a plan with a device batch == 0
 * returns GVTM_OK. */
int gvtm_synthesize_targets_voices_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists,
		const int32_t* d_list_ids, const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts,
		const int32_t* d_voice_ids, size_t batch, size_t max_steps, float* d_audio, size_t audio_stride,
		int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream);

/* gvtm_synthesize_targets_device for reference model 5, as the interactive window runs it: one-voice plans of
 * gvtm_plan_create_model5 (VocalTractModel5<double,1>) and gvtm_plan_create_model5_float (VocalTractModel5<float,1>).
 * Every argument, the statuses 0 to 4 and the sample counts (gvtm_targets_output_count / _capacity) are that entry's.
 * The rule for model 5: utterance b's samples are those of VocalTractModel5<T,1>(config, interactive = true) fed
 * v[s][0..16) of gvtm_targets_apply_host by setParameter before step s, s = 0 .. S_b - 1, then finishSynthesis(): in the
 * float class bit for bit, in the double class within the model 5 parity bar.  They are therefore NOT those of
 * gvtm_synthesize_batch_device on the same frames at one step per frame: a model constructed for the interactive window
 * divides each step's tube output by that step's fundamental frequency before the sample-rate converter
 * (vtm/VocalTractModel5.h:579, compensating the difference filter at the output), which the batch protocol's model does not.
 * Enqueue-only: the check kernel and the synthesis launch on hip_stream, nothing else.  The call uses the plan's step-count
 * scratch: calls on one plan must be ordered on one stream.  Refused before any device work, in this order: a null plan;
 * with batch > 0 what gvtm_synthesize_targets_device refuses (GVTM_ERR_INVALID_ARGUMENT); a plan of several voices or a
 * plan of the models 0 to 4, which have gvtm_synthesize_targets_device (GVTM_ERR_UNSUPPORTED); a design-only plan
 * (GVTM_ERR_NO_DEVICE), with batch == 0 too; on a plan with a device batch == 0 returns GVTM_OK.  The same as a session:
 * gvtm_stream_push_targets_model5 ("Streams fed parameter targets" below).  Model 5 targets under several voices:
 * gvtm_synthesize_targets_model5_voices_device (next). */
int gvtm_synthesize_targets_model5_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts, size_t batch,
		size_t max_steps, float* d_audio, size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status,
		void* hip_stream);

/* gvtm_synthesize_targets_model5_device with a voice id per utterance: one articulator trajectory under every model 5 speaker
 * in one launch, although the five voice variants' tract lengths, and with them their internal rates and their N, differ by
 * more than a factor of two.  Argument for argument it is gvtm_synthesize_targets_voices_device:
 *   d_voice_ids [batch] int32                    utterance b walks its lists under voice d_voice_ids[b] of the plan: that
 *                                                voice's own N = gvtm_targets_filter_length(plan, voice) and 1 / N.  Lists
 *                                                hold no N, so utterances of different voices may share a list
 *   d_audio [batch][audio_stride]                utterance b yields gvtm_targets_voice_output_count(plan, voice_b, S_b) samples
 *   every other argument                         as gvtm_synthesize_targets_device's
 * Plans of gvtm_plan_create_model5_voices and gvtm_plan_create_model5_float_voices of any number of voices, and a one-voice
 * gvtm_plan_create_model5 plan, on which ids that are all 0 give gvtm_synthesize_targets_model5_device's bytes.  In both
 * classes voice v's utterances come out bit for bit -- samples, out_counts, maxabs -- as gvtm_synthesize_targets_model5_device
 * synthesizes them on a one-voice plan made from configs[v]: the samples are the interactive model's (divided by f0), in the
 * float class the reference's VocalTractModel5<float,1>(config, interactive = true) bit for bit, in the double class within the
 * model 5 parity bar.  It is an entry of its own for that reason, as gvtm_synthesize_targets_model5_device is.  A voice id
 * outside [0, n_voices) is status 5 (above: looked at first, out_counts -1, maxabs 0, the audio row untouched); an utterance
 * refused with status 1 to 4 is one of 0 steps of its voice.  Enqueue-only: the check kernel, the grouping kernel of
 * gvtm_synthesize_voices_device and the synthesis launch on hip_stream, nothing else.  The call uses the plan's grouping
 * scratch and step-count scratch: calls on one plan must be ordered on one stream.  Refused before any device work, in this
 * order: a null plan; with batch > 0 what gvtm_synthesize_targets_device refuses, NULL d_voice_ids, a stride below
 * gvtm_targets_voices_output_capacity(plan, max_steps) (GVTM_ERR_INVALID_ARGUMENT); a plan of the models 0 to 4, which have
 * gvtm_synthesize_targets_voices_device (GVTM_ERR_UNSUPPORTED); a gvtm_plan_create_model5_float plan, which has no launch of
 * several voices (GVTM_ERR_UNSUPPORTED); a design-only plan (GVTM_ERR_NO_DEVICE), with batch == 0 too; on a plan with a
 * device batch == 0 returns GVTM_OK.  Not available: streams of targets under several voices, in either model family. */
int gvtm_synthesize_targets_model5_voices_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists,
		const int32_t* d_list_ids, const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts,
		const int32_t* d_voice_ids, size_t batch, size_t max_steps, float* d_audio, size_t audio_stride,
		int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream);

/*
 * Streams fed parameter targets: the interactive window as a session.  Targets arrive while the audio is playing, so a
 * stream of gvtm_stream_create takes them push by push; the filters run in the synthesis kernel and their 16 sums travel in
 * the utterance's device state.  All pointers are HOST memory, as gvtm_stream_push's.
 *   list_offsets [16 * batch + 1]   utterance b's parameter p owns the points [off[16b+p], off[16b+p+1]) of point_steps /
 *                                   point_values.  Their steps count from the first step THIS push adds for the utterance:
 *                                   a point at step 0 takes effect on the push's first step
 *   step_counts [batch] or NULL     the steps utterance b advances by; NULL: all max_steps.  0 is allowed
 *   audio, audio_stride, out_counts as gvtm_stream_push; audio_stride comes from gvtm_stream_targets_capacity
 *   status_out [batch] or NULL      out: the statuses of gvtm_targets_apply_host
 * A push synthesizes the steps that fit the serial wavefronts' granule of 12 steps and keeps the rest (at most 11) pending;
 * no look-ahead step is kept, since a step does not interpolate towards a successor.  gvtm_stream_finish synthesizes the
 * pending steps and flushes.  Contract: an utterance's steps pushed in any grouping over any number of calls and then
 * finished give, in every precision bit for bit, the samples, sample count and maxabs of one gvtm_synthesize_targets_device
 * call on the whole utterance's lists.
 *
 * The stream keeps, per utterance and parameter, the points the rule from any step (gvtm_targets_apply_host_from) still
 * needs, on the host and in absolute steps: a push appends its points, a launch uploads what is held (8 bytes a point), and
 * what the rule allows is forgotten.  gvtm_stream_targets_points reports the points held per utterance: never more than the
 * points of the last N + 12 steps plus 16, however long the session.
 *
 * gvtm_stream_targets_capacity is the row length for any push or finish that adds up to max_new_steps steps: the new steps,
 * 11 pending ones, the flush with its overrun lap, and one more sample.  (size_t)-1 on a null stream.
 *
 * Checked on the host before anything is launched; the first that applies: a null stream (GVTM_ERR_INVALID_ARGUMENT); a
 * stream of a plan of several voices or of a model 5 plan (GVTM_ERR_UNSUPPORTED: the one-shot entry takes neither; model 5
 * has gvtm_stream_push_targets_model5, several voices gvtm_stream_push_targets_voices, both below); then,
 * all GVTM_ERR_INVALID_ARGUMENT, a finished stream; a stream fed frames or event lists since its last reset; a null
 * list_offsets; a max_steps beyond the step counter; points without their tables; an utterance that is refused -- status 1
 * for a count outside [0, max_steps], 2, 3 and 4 as above, and 4 also for a point whose step is at or beyond the
 * utterance's count in this push -- in which case status_out says which; more than 2^31 internal steps since the reset; an
 * audio_stride smaller than the call produces or a null audio with samples due.  A refused call leaves the stream exactly
 * as it found it: no utterance has advanced, and the corrected call synthesizes nothing twice.
 *
 * One feed per run, as with frames and event lists: gvtm_stream_push and gvtm_stream_push_events refuse a targets-fed stream
 * and gvtm_stream_push_targets a frames-fed or events-fed one until the next gvtm_stream_reset, which also clears the held
 * points, the pending steps and the sums.
 */
int gvtm_stream_push_targets(gvtm_stream* stream, const int64_t* list_offsets, const int32_t* point_steps,
		const float* point_values, const int32_t* step_counts, size_t max_steps, float* audio, size_t audio_stride,
		int64_t* out_counts, int32_t* status_out);
/* gvtm_stream_push_targets for reference model 5, the model the interactive window constructs: streams of gvtm_stream_create
 * on the one-voice plans of gvtm_plan_create_model5 and gvtm_plan_create_model5_float.  Every argument is that entry's.  An
 * entry of its own for the reason gvtm_synthesize_targets_model5_device is one: the samples are those of the model
 * constructed with interactive = true, which divides each step's signal by that step's f0 -- not those of a frames-fed
 * stream of the same plan.
 * Model 5's serial stages work in blocks of four steps: a push synthesizes the steps that fit a granule of 4 and keeps the
 * rest (at most 3) pending.  Contract: an utterance's steps pushed in any grouping over any number of calls and then
 * finished give, in both classes bit for bit, the samples, sample count and maxabs of one
 * gvtm_synthesize_targets_model5_device call on the whole utterance's lists: in the float class the reference's interactive
 * model bit for bit, in the double class within the model 5 parity bar.
 * gvtm_stream_finish, gvtm_stream_reset, gvtm_stream_targets_points and gvtm_stream_targets_capacity serve such a stream as
 * they are: the capacity's 11 pending steps and the bound on the points held (those of the last N + 12 steps plus 16) hold
 * with room to spare.
 * Refused, the first that applies: a null stream (GVTM_ERR_INVALID_ARGUMENT); a stream of a plan of several voices or of a
 * plan of the models 0 to 4, which have gvtm_stream_push_targets (GVTM_ERR_UNSUPPORTED); then everything
 * gvtm_stream_push_targets refuses, in its order and with its status codes, and a refused call leaves the stream exactly as
 * it found it.  One feed per run here too: gvtm_stream_push and gvtm_stream_push_events refuse a model 5 stream fed targets,
 * this entry one fed frames or event lists, until the next gvtm_stream_reset; after a reset the stream takes either feed. */
int gvtm_stream_push_targets_model5(gvtm_stream* stream, const int64_t* list_offsets, const int32_t* point_steps,
		const float* point_values, const int32_t* step_counts, size_t max_steps, float* audio, size_t audio_stride,
		int64_t* out_counts, int32_t* status_out);
/* The two entries above under a mix of voices: streams of gvtm_stream_create_voices on a plan of several voices, utterance b
 * spoken by the stream's own voice of it (the ids of gvtm_stream_create_voices or of the last gvtm_stream_reset_voices; no
 * id travels with a push).  gvtm_stream_push_targets_voices takes plans of the models 0 to 4 in every precision,
 * gvtm_stream_push_targets_model5_voices the plans of gvtm_plan_create_model5_voices and
 * gvtm_plan_create_model5_float_voices; each takes the arguments of gvtm_stream_push_targets, argument for argument, and also
 * a stream of a one-voice plan of its family, on which it is bit for bit the one-voice entry above (the two may alternate
 * within a run).  Every utterance walks its lists through the filter of its own voice (gvtm_targets_filter_length(plan, v):
 * the voices' internal rates differ, and so do their lengths); the granules stay the stream's, 12 steps resp. 4.
 * Contract: for every voice v, the steps of an utterance of voice v pushed in any grouping over any number of calls and
 * then finished give, bit for bit in every precision resp. both classes, the samples, sample count and maxabs of one
 * gvtm_synthesize_targets_voices_device resp. gvtm_synthesize_targets_model5_voices_device call on the whole lists under
 * voice v -- so the float class of model 5 stays the reference's interactive model bit for bit under every voice.
 * gvtm_stream_finish, gvtm_stream_reset, gvtm_stream_reset_voices (the next run walks the new voices' filters),
 * gvtm_stream_listen with its take and peek entries and gvtm_stream_targets_points serve such a stream; the points held for
 * utterance b never exceed those of its last N_v + 12 steps plus 16, N_v its own voice's length.
 * gvtm_stream_targets_capacity answers the largest count over ALL the plan's voices, whichever the ids name, so that
 * gvtm_stream_reset_voices never invalidates a stride (on a one-voice plan: the value it always had).
 * Refused, the first that applies: a null stream (GVTM_ERR_INVALID_ARGUMENT); a stream of the other model family
 * (GVTM_ERR_UNSUPPORTED); then everything gvtm_stream_push_targets refuses, in its order and with its status codes, and a
 * refused call leaves the stream exactly as it found it.  The two one-voice entries above keep refusing a plan of several
 * voices. */
int gvtm_stream_push_targets_voices(gvtm_stream* stream, const int64_t* list_offsets, const int32_t* point_steps,
		const float* point_values, const int32_t* step_counts, size_t max_steps, float* audio, size_t audio_stride,
		int64_t* out_counts, int32_t* status_out);
int gvtm_stream_push_targets_model5_voices(gvtm_stream* stream, const int64_t* list_offsets, const int32_t* point_steps,
		const float* point_values, const int32_t* step_counts, size_t max_steps, float* audio, size_t audio_stride,
		int64_t* out_counts, int32_t* status_out);
size_t gvtm_stream_targets_capacity(const gvtm_stream* stream, size_t max_new_steps);
/* held_out [batch] (host): the points the stream holds for each utterance */
int gvtm_stream_targets_points(const gvtm_stream* stream, int64_t* held_out);

/*
 * Streams fed event lists.  The reference produces an utterance chunk by chunk (one generateOutput() per /c chunk,
 * Controller.cpp:141-154); a stream takes the next chunk or chunks of each of its utterances as they are parsed, generates
 * their frames on the device straight behind the frames it still holds, synthesizes what can be synthesized and returns
 * the new samples.  The frames never leave the device, and the drift generators (one per utterance) live in the stream.
 *
 * gvtm_stream_push_events works on every stream of gvtm_stream_create and gvtm_stream_create_voices (models 0 to 4 in every
 * precision, model 5 in both classes, one voice or several) whose plan has track configurations
 * (gvtm_plan_set_voice_tracks, which takes a one-voice plan too); utterance b is generated under the configuration of its
 * stream voice.
 *   events, chunk_offsets [n_chunks + 1], utt_chunks [batch + 1]
 *                     HOST memory: the two offset tables of gvtm_generate_tracks_chunks_device.  Utterance b receives the
 *                     chunks [utt_chunks[b], utt_chunks[b+1]) -- none is allowed, and a NULL utt_chunks gives no utterance
 *                     a chunk; n_chunks = utt_chunks[batch].
 *   frame_counts_out  [batch] int32 (may be NULL): the frames this call generated per utterance
 *   audio, audio_stride, out_counts: as gvtm_stream_push.  audio_stride comes from gvtm_stream_capacity(stream, n), n the
 *                     largest per-utterance frame total of the push (gvtm_tracks_chunks_frame_count on the host).
 * Each chunk is generated exactly as gvtm_generate_tracks_chunks_device generates it: a list of its own; fewer than two
 * events yield nothing and leave the drift state alone; the drift state a chunk leaves is the next chunk's, within a push
 * and from push to push.  The new frames go behind the utterance's held frames, and the push then does what
 * gvtm_stream_push does.  gvtm_stream_finish and gvtm_stream_capacity take such a stream as they are.  Contract: an
 * utterance's chunks pushed in any grouping over any number of calls and then finished give, bit for bit and in every
 * precision, the samples, sample count, maxabs, total frame count and final drift state of one
 * gvtm_synthesize_events_chunks_device call on the whole utterance with the same voice and the same initial drift state.
 *
 * One feeding mode per run: between two resets a stream is fed frames (gvtm_stream_push), event lists or parameter targets
 * (gvtm_stream_push_targets, gvtm_stream_push_targets_model5 or their _voices forms, above), never two of them; once one entry has been used the others return
 * GVTM_ERR_INVALID_ARGUMENT until the next reset, and so does
 * gvtm_stream_set_drift between a gvtm_stream_push_events and the next reset.
 *
 * The drift generators: gvtm_stream_create* starts every one fresh ({0.7892347, 0, 0, 0, 0}).  gvtm_stream_reset and
 * gvtm_stream_reset_voices leave them as they are (the reference's Controller resets its model for every utterance and
 * never reseeds its generator); gvtm_stream_set_drift(stream, NULL) is what reseeds them.
 *
 * Refused with GVTM_ERR_INVALID_ARGUMENT, in this order and before any device work: a null stream; a finished stream; a
 * stream fed frames or targets since its last reset; a plan without track configurations; null events or chunk_offsets while chunks
 * are present; offsets that decrease or are negative; more frames than one push can hold; an audio_stride smaller than the
 * call produces, or a null audio with samples due (the host counts every frame and sample in advance); more than 2^31
 * internal steps since the reset.  A call refused here leaves the stream exactly as it found it: held frames, drift states
 * and feeding mode.  A device error after the tracks launch leaves the stream finished (pushes refused) until a reset.
 * Synchronous; the tracks kernel, the synthesis launch and the kernel that moves the kept frames to the front of the
 * stream's frame buffer run in this order on the stream's launch stream.
 */
int gvtm_stream_push_events(gvtm_stream* stream, const gvtm_event* events, const int64_t* chunk_offsets,
		const int64_t* utt_chunks, float* audio, size_t audio_stride, int64_t* out_counts, int32_t* frame_counts_out);
/* the stream's drift generators, one per utterance */
int gvtm_stream_get_drift(const gvtm_stream* stream, gvtm_drift_state* states_out /* [batch], host */);
/* states [batch] (host), or NULL: fresh generators -- the one call that reseeds them */
int gvtm_stream_set_drift(gvtm_stream* stream, const gvtm_drift_state* states);

/*
 * Event lists in from host memory, packed samples out: what Controller::synthesizePhoneticStringToFile does for one
 * utterance (Controller.cpp:194-200: the /c chunks' event lists in, the int16 samples out, and with vtmParamFile the
 * parameter list it synthesized), for a whole ragged batch in one call.  The packed host entries above ("Ragged batches")
 * with event lists in the place of frames: the frames are generated on the device and never cross PCIe unless the caller
 * asks for them, and what is staged on the device is bounded by a slice.  For callers that do not link HIP.
 *
 * All arguments are host memory.
 *   events, chunk_offsets [n_chunks + 1], utt_chunks [batch + 1]
 *                      the two offset tables of gvtm_generate_tracks_chunks_device; here both must start at 0 and must not
 *                      decrease; n_chunks = utt_chunks[batch].  The track configurations are the plan's
 *                      (gvtm_plan_set_voice_tracks, which takes a one-voice plan too).
 *   voice_ids          [batch], or NULL on a one-voice plan: the synthesis then goes through the single-voice launch, as in
 *                      the packed entry (so a gvtm_plan_create_model5_float plan takes NULL ids only; the tracks kernel
 *                      is given zeros)
 *   frames of utterance b = the sum over its chunks of gvtm_tracks_frame_count (the host walks the lists, as
 *                      gvtm_stream_push_events does); frame_offsets = their prefix sum; the sample offsets are exactly
 *                      gvtm_packed_sample_offsets of those frame offsets.  No utterance is cut: there is no max_frames.
 *   audio / pcm, sample_offsets_out, out_counts, maxabs, scales
 *                      as gvtm_synthesize_packed_host* returns them: gaps are zeros, nothing beyond offset[batch] is touched
 *   frame_offsets_out  [batch+1] (may be NULL)
 *   frames_out         [frame_offsets[batch]][16] float32 (may be NULL), frames_capacity in frames: the frames that were
 *                      synthesized, packed, in the layout gvtm_synthesize_packed_host takes as input (the reference's
 *                      vtmParamFile, Controller.cpp:198, `gama_tts tts -p`)
 *   drift              [batch] in/out as in the device entries; NULL: a fresh generator per utterance, nothing returned
 *
 * Contract.  Against gvtm_synthesize_events_chunks_device on the same plan, with the same ids and initial drift states and
 * max_frames at least the longest utterance: every utterance's samples, sample count, maxabs, frame count and final drift
 * state are bit for bit that call's, in every precision, for the models 0 to 4 and both classes of model 5, one voice or
 * several.  The int16 samples and scales are bit for bit those of gvtm_synthesize_packed_host_pcm16 fed frames_out, and
 * frames_out is bit for bit what gvtm_generate_tracks_chunks_device generates.
 *
 * Refused in this order, before any device work, with GVTM_ERR_INVALID_ARGUMENT unless another status is named: a null plan;
 * a plan without track configurations; a null table; null events while chunks are present; tables that do not start at 0 or
 * that decrease; the ids, as the packed entry checks them; an utterance whose frames x control_steps does not fit the 31-bit
 * step counter; a null audio / pcm buffer; a capacity below the layout's (audio_capacity / pcm_capacity, and
 * frames_capacity when frames_out is given); a design-only plan: GVTM_ERR_NO_DEVICE; batch == 0: GVTM_OK.  A refused call
 * writes nothing to any output array.
 *
 * Slices, as the packed entries': three staging sets deep on the plan's three streams,
 *   H2D events + tracks kernel(i+1) || synthesis + pack(i) || D2H packed output [+ packed frames](i-1)
 * (the tracks kernel is queued behind its slice's events on the H2D stream: its walk is as long as the slice's longest list,
 * and there it runs as the compute units of the slice before come free instead of in front of its own synthesis launch).
 * The events of a slice are one contiguous range of `events`; the two tables, the ids and the drift states are the batch's,
 * uploaded once.  A slice of n utterances, the longest of F frames, holds in its set its events (sizeof(gvtm_event) = 296;
 * the rows behind them are stored 16 bytes at a time), its padded frames, its padded float samples, its packed output and,
 * with frames_out, its packed frames:
 *   set_bytes = round_up(296 * events_of_slice, 64) + 64 * n * F + 4 * n * S + w * aligned_samples_of_slice
 *               (+ 64 * frames_of_slice with frames_out)                    (S and w as for the packed entries)
 * The sets are the packed entries' own three: gvtm_plan_set_staging_limit and gvtm_plan_packed_stats govern and report
 * these calls as they do those, slices are closed by the same rule, an utterance that does not fit a set on its own refuses
 * the call with GVTM_ERR_OUT_OF_MEMORY (the message gives the bytes it needs), and the packed and the events-packed entries
 * may not overlap each other on one plan.  Synchronous.  After the last slice the frame counts of the device are compared
 * with the host's; a difference is an internal error (GVTM_ERR_HIP).
 */

/* The layout alone.  Host only, works on GVTM_DEVICE_NONE plans; the tables are checked as the synthesis entries check them
 * (up to the 31-bit counter).  Returns the capacity in samples, sample_offsets_out[batch]; (size_t)-1 on a bad argument,
 * with nothing written. */
size_t gvtm_events_packed_layout(const gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets,
		const int64_t* utt_chunks, const int32_t* voice_ids, size_t batch,
		int64_t* frame_offsets_out /* [batch+1] or NULL */, int64_t* sample_offsets_out /* [batch+1] or NULL */);

int gvtm_synthesize_events_packed_host(gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets,
		const int64_t* utt_chunks, const int32_t* voice_ids, size_t batch, float* audio, size_t audio_capacity,
		int64_t* sample_offsets_out, int64_t* frame_offsets_out, float* frames_out, size_t frames_capacity,
		int64_t* out_counts, float* maxabs, gvtm_drift_state* drift);
/* The same ending as gvtm_synthesize_packed_host_pcm16 ends; scales [batch] may be NULL. */
int gvtm_synthesize_events_packed_host_pcm16(gvtm_plan* plan, const gvtm_event* events, const int64_t* chunk_offsets,
		const int64_t* utt_chunks, const int32_t* voice_ids, size_t batch, int16_t* pcm, size_t pcm_capacity,
		int64_t* sample_offsets_out, int64_t* frame_offsets_out, float* frames_out, size_t frames_capacity,
		int64_t* out_counts, float* maxabs, float* scales, gvtm_drift_state* drift);

/* Same with host buffers (H2D, kernel, D2H, synchronous). */
int gvtm_generate_tracks_host(int device, const gvtm_track_config* config, const gvtm_event* events,
		const int64_t* event_offsets, size_t batch, size_t max_frames, float* params, int32_t* frame_counts,
		gvtm_drift_state* drift);

/*
 * Spectrum analysis: the listening half of the editor's interactive window.  There every output sample also goes into a
 * ring of 65 536 samples (InteractiveAudio.cpp:146-158, 192-205), and AnalysisWindow::showData (AnalysisWindow.cpp:189-300)
 * turns each full ring into the picture the user watches while moving the sliders.  Here: for a whole batch, on the audio
 * rows and out_counts every synthesis entry leaves on the device, so that a closed loop compares a few thousand bins and
 * not 256 KB of samples per buffer.
 *
 * The rule, for one buffer s[0 .. 65536) of float samples:
 *   1. peak      maxValue = the largest |s[i]| over all 65 536 samples, not only the window's.  maxValue > 0: normCoef =
 *                (float)(1.0 / (double)maxValue) and s[i] = s[i] * normCoef (a float product); 0: the samples stay.
 *   2. signal    the window's "Signal" view: the first W normalised samples, unwindowed.
 *   3. spectrum  x[i] = (float)((double)s[i] * window[i]) for i < W and 0 behind; X = the 65 536-point real DFT of x in
 *                float; mag[i] = sqrt(re^2 + im^2) / 256; linear: mag[i]; log: 20 log10(mag[i]), min_db where that is
 *                below min_db (an empty bin, log10(0) = -inf, is min_db); the bins 0 .. n_bins - 1, n_bins the first i with
 *                i * ((double)sample_rate / 65536) > max_freq_hz, else 32 769; max_freq_hz <= 0: all 32 769.
 *   4. buffers   an utterance's buffers are consecutive and complete, as the ring hands them over: buffer k is the samples
 *                [first + 65536 k, first + 65536 (k + 1)); min(max_buffers, floor((count - first) / 65536)) are analysed,
 *                none if first > count (or first < 0).
 * The window scales its output by a running peak before it reaches the ring; step 1 removes any constant scale, so these
 * entries take the unscaled samples the synthesis entries write.
 * Steps 1 and 2 are the reference's bit for bit.  The float DFT is not FFTW's bit for bit (float transforms differ by their
 * factorisation): the yardstick is the double DFT of the same x, which the device's float transform (twiddles from one
 * table designed in double) and the host's restatement (a double transform rounded to float at the end) both approximate;
 * tests/analysis_cases.py gives the bars.  Measured: profiles/analysis_ab.md.
 */
#define GVTM_ANALYSIS_FFT_SIZE 65536
#define GVTM_ANALYSIS_MAX_BINS 32769
#define GVTM_ANALYSIS_DEFAULT_BUFFERS 128 /* what gvtm_analysis_create reserves on a device: 64 MB of scratch, which stays
                                             in the device's caches; batches of thousands of buffers run some 10 % faster
                                             with gvtm_analysis_reserve(1024), 512 MB */
#define GVTM_WINDOW_RECTANGULAR 0 /* AnalysisWindow.cpp's order (WINDOW_RECTANGULAR ...) */
#define GVTM_WINDOW_TRIANGULAR 1
#define GVTM_WINDOW_HANN 2
#define GVTM_WINDOW_HAMMING 3
#define GVTM_WINDOW_BLACKMAN 4

/* window_size: a power of two in [32, 65536]; log_scale: 0 linear, otherwise log; sample_rate: Hz, not 0.  Anything else
 * (a NaN min_db or max_freq_hz included) is GVTM_ERR_INVALID_ARGUMENT. */
struct gvtm_analysis_config {
	int32_t window_type;
	int32_t window_size;
	int32_t log_scale;
	double min_db;
	double max_freq_hz;
	uint32_t sample_rate;
};
typedef struct gvtm_analysis_config gvtm_analysis_config;
typedef struct gvtm_analysis gvtm_analysis;

/* Designs the window (the reference's five formulas in double, on the host) and counts the bins; on a device it also
 * uploads the window and the twiddle table and reserves scratch for GVTM_ANALYSIS_DEFAULT_BUFFERS buffers in flight.
 * device GVTM_DEVICE_NONE: a design-only object, whose device entry returns GVTM_ERR_NO_DEVICE, as plans do. */
int gvtm_analysis_create(int device, const gvtm_analysis_config* config, gvtm_analysis** analysis_out);
void gvtm_analysis_destroy(gvtm_analysis* analysis);
/* n_bins; (size_t)-1 for a null object */
size_t gvtm_analysis_bin_count(const gvtm_analysis* analysis);
/* the window's W doubles; capacity in doubles */
int gvtm_analysis_window(const gvtm_analysis* analysis, double* window_out, size_t capacity);
/* step 4: the buffers analysed of an utterance of n_samples samples */
size_t gvtm_analysis_buffer_count(int64_t n_samples, int64_t first_sample, size_t max_buffers);
/* Device scratch for n_buffers (>= 1) buffers in flight: 512 KB each, the two intermediate images of the transform, which
 * at the default stay in the device's caches.  Synchronous (it waits for the device before it frees the old scratch); the
 * one place an allocation happens after creation.  A batch with more buffers than reserved runs in slices over the same
 * scratch, one after the other on the caller's stream, with the same results. */
int gvtm_analysis_reserve(gvtm_analysis* analysis, size_t n_buffers);
/* The rule on the host for one utterance, the DFT a plain double transform rounded to float at the end: the restatement
 * the tests pin, not a fast path.  samples [n_samples]; spectra_out [max_buffers][n_bins] or NULL; signal_out
 * [max_buffers][W] or NULL (not both); n_buffers_out (may be NULL): the buffers analysed; rows behind them are left
 * untouched.  Works on a design-only object. */
int gvtm_analysis_apply_host(const gvtm_analysis* analysis, const float* samples, size_t n_samples, size_t first_sample,
		size_t max_buffers, float* spectra_out, float* signal_out, size_t* n_buffers_out);
/* The rule for a batch on the device, enqueue-only on hip_stream: it allocates nothing, copies nothing synchronously and
 * never waits, so it may follow a synthesis entry on the same stream without synchronisation in between.
 *   d_audio, audio_stride   float [batch][audio_stride]: the rows a synthesis entry wrote
 *   d_counts                int64 [batch]: the samples of each row (a synthesis entry's out_counts); a count above
 *                           audio_stride is taken as audio_stride
 *   d_first                 int64 [batch], or NULL for 0: each utterance's first analysed sample; any index, odd ones too
 *   d_spectra               float [batch][max_buffers][n_bins], or NULL
 *   d_signal                float [batch][max_buffers][W], or NULL
 *   d_buffers_out           int32 [batch] (may be NULL): gvtm_analysis_buffer_count of each utterance
 * Rows of d_spectra and d_signal behind an utterance's buffer count are left untouched.  Calls on one object must be
 * ordered on one stream (they share its scratch).
 * Refused with GVTM_ERR_INVALID_ARGUMENT: a null object; with batch > 0 and max_buffers > 0, null d_audio or d_counts, both
 * outputs null, or batch * max_buffers above 2^31.  A design-only object: GVTM_ERR_NO_DEVICE.  batch or max_buffers 0:
 * GVTM_OK (d_buffers_out is then zeroed for max_buffers 0). */
int gvtm_analyze_spectrum_device(gvtm_analysis* analysis, const float* d_audio, size_t audio_stride, const int64_t* d_counts,
		const int64_t* d_first, size_t batch, size_t max_buffers, float* d_spectra, float* d_signal,
		int32_t* d_buffers_out, void* hip_stream);

/*
 * Streams that listen: the two halves of the interactive window in one object.  In the reference
 * InteractiveAudio::Processor::process writes every output sample into the analysis ring as it is produced
 * (InteractiveAudio.cpp:146-158, 192-205) and the window reads the ring whenever it is full (AnalysisWindow.cpp:199-225).
 * gvtm_stream_listen gives a stream that ring, on the device, for every utterance of its batch: each push then leaves the
 * spectra (and signal views) of the rings it completed in a queue on the device, and need not return audio at all.
 *
 * The rule (the ring hands over consecutive, complete buffers: step 4 of the analysis rule above):
 *   - an utterance's samples since the stream's last reset are numbered from 0, in the order the pushes and the finish
 *     return them; its buffer k is the samples [65536 k, 65536 (k + 1));
 *   - a buffer is analysed when the launch that brings its last sample has run;
 *   - an incomplete ring is never analysed, not at gvtm_stream_finish either: the window shows nothing until the ring is full.
 * Two things the reference does are deliberately not reproduced:
 *   - the JACK ring drops samples while the GUI timer has not yet consumed a full ring; here no sample is dropped;
 *   - the window scales samples by its running peak before they reach the ring.  Step 1 of the analysis rule removes a
 *     constant scale; the running one depends on JACK's period size, so it is not a property of the model.
 * Contract: utterance b's queued spectra and signal views, fed in any grouping by any of the stream's feeds, are bit for bit
 * the rows k of what gvtm_analyze_spectrum_device writes for the same analysis object with first = 0 on the utterance's whole
 * sample sequence (the pushes' and the finish's samples concatenated) -- where the stream contract makes those samples
 * bit-identical to the one-shot entry's, on that entry's row.  The arithmetic of the analysis does not depend on where a
 * buffer lies or how it is aligned; only the width of the loads does.
 *
 * A listening stream is taken as it is by every push entry (gvtm_stream_push, _push_events, _push_targets,
 * _push_targets_model5, _push_targets_voices, _push_targets_model5_voices) and by gvtm_stream_finish, whatever its voices, model and precision.  On it `audio` may be NULL although
 * samples are due: audio_stride is then ignored, out_counts is still filled, and no sample leaves the device.  One refusal is
 * added, behind the entry's own and before anything is launched or kept: a call that would complete more buffers than an
 * utterance's queue has room for is GVTM_ERR_INVALID_ARGUMENT and leaves the stream exactly as found; the same call succeeds
 * after gvtm_stream_take_spectra.  (Every sample count is known before the launch: gvtm_listen_buffer_count.)
 * gvtm_stream_reset and _reset_voices empty rings and queues and keep the listener; gvtm_stream_destroy frees them.  A stream
 * that does not listen is what it has always been: no kernel, allocation or upload is added to its launches, and a NULL
 * audio with samples due is refused.
 * The analysis object must outlive the listener.  Calls on streams that share one analysis object must not overlap: they
 * share its scratch.  A launch analyses the rings it completes in slices of the object's reserved scratch
 * (gvtm_analysis_reserve), as the one-shot entry does.
 */
#define GVTM_LISTEN_SPECTRA 1
#define GVTM_LISTEN_SIGNAL 2

/* The rule's arithmetic: the buffers completed by n_new more samples on a ring holding `fill` samples, and in *fill_after
 * (may be NULL) what the ring holds afterwards.  A fill outside [0, 65536) or a negative n_new: 0, the fill unchanged. */
size_t gvtm_listen_buffer_count(int64_t fill, int64_t n_new, int64_t* fill_after);
/* Allocates on the stream's device a ring of 65 536 floats per utterance and, for the views asked for (GVTM_LISTEN_*, or'ed),
 * a queue of max_buffers analysed buffers per utterance.  Called again on a fresh stream it replaces the listener.
 * GVTM_ERR_INVALID_ARGUMENT: null arguments, max_buffers 0, views 0 or with unknown bits, an analysis object on another
 * device than the stream's plan, an analysis sample_rate that is not the output_rate of every voice of the plan, a stream
 * fed since its last reset (the ring starts with the utterance).  GVTM_ERR_NO_DEVICE: a design-only analysis object.
 * GVTM_ERR_OUT_OF_MEMORY: a failed allocation; the stream is left not listening. */
int gvtm_stream_listen(gvtm_stream* stream, gvtm_analysis* analysis, size_t max_buffers, int views);
/* Frees the rings and queues; allowed at any time.  The stream then synthesizes on as one that never listened. */
int gvtm_stream_unlisten(gvtm_stream* stream);
/* The samples in each ring and the buffers queued (either may be NULL). */
int gvtm_stream_listen_state(const gvtm_stream* stream, int64_t* fill_out /* [batch] */, int32_t* queued_out /* [batch] */);
/* Copies utterance b's queued buffers to the rows 0 .. queued[b] - 1 of its block of the host arrays and leaves the rows behind
 * them untouched, writes the counts to buffers_out and empties the queues.  With both arrays NULL it only empties.  A
 * non-null array of a view not asked for at gvtm_stream_listen: GVTM_ERR_INVALID_ARGUMENT. */
int gvtm_stream_take_spectra(gvtm_stream* stream, float* spectra /* [batch][max_buffers][n_bins] host, or NULL */,
		float* signal /* [batch][max_buffers][W] host, or NULL */, int32_t* buffers_out /* [batch], or NULL */);
/* Hands out the queues where they lie on the device, in the layout of take (NULL for a view not kept), and a device table
 * of the queued counts, for loops whose comparison runs on the device.  Empties nothing.  The pointers stay valid until the
 * next call on the stream.  Any of the three may be NULL. */
int gvtm_stream_peek_spectra_device(const gvtm_stream* stream, const float** d_spectra, const float** d_signal,
		const int32_t** d_queued);

/* ---------------------------------------------------------------------------------------------
 * Event lists from posture sequences: the step in front of everything above.  Replaces
 * EventList::generateEventList() / applyRule() / createSlopeRatioEvents() / insertEvent() / setZeroRef()
 * (vtm_control_model/EventList.cpp:302-371, 373-432, 435-676) for a batch: per phone a posture id, a marked bit and two
 * tempos in, gvtm_event lists out, in the layout every events entry above reads, never leaving the device.  The rule
 * data and the posture onsets that EventList::applyIntonation() places its points by come out beside them.
 * Bit-identical to the reference's list (the debug `flag` of an event is not kept).
 *
 * The articulatory database arrives compiled to flat arrays (gama_tts_amd/control_model.py compiles an artic.xml;
 * INTEGRATION.md tells how a GamaTTS build fills them from its Model).  Every number is held in the type the reference
 * holds it in.  (The three structures of this section are declared in two steps, `struct X {...}; typedef struct X X;`.)
 */

/* The compiled model: host arrays, read during gvtm_rules_create only. */
struct gvtm_rules_model {
	int32_t n_postures, n_rules, n_equations, n_program_ops, n_transitions, n_items, n_points, n_slopes;
	/* postures */
	const float* param_target;    /* [n_postures][16] Posture::getParameterTarget */
	const float* symbol_target;   /* [n_postures][6] transition, qssa, qssb, marked transition, marked qssa, marked qssb
	                                 (Rule::evaluateExpressionSymbols, Rule.cpp:468-548) */
	const float* param_min;       /* [16] Parameter::minimum() */
	const float* param_max;       /* [16] */
	/* rules, in database order */
	const int32_t* rule_n_expr;   /* [n_rules] boolean expressions: 2, 3 or 4, which is also the rule's type */
	const int32_t* rule_equations;          /* [n_rules][5] equations of rd, beat, mark1, mark2, mark3; -1: none */
	const int32_t* rule_param_transition;   /* [n_rules][16] */
	const int32_t* rule_special_transition; /* [n_rules][16], -1: none; points only */
	const uint8_t* match;         /* [n_rules][4][n_postures] bit 0: the position's expression holds for the posture
	                                 unmarked, bit 1: marked */
	/* equations: postfix programs.  program_op: the operation in the low byte -- 0 push program_const[i], 1 push the
	 * FormulaSymbol (op >> 8) (FormulaSymbol.h:36-60), 2 negate, 3 add, 4 subtract, 5 multiply, 6 divide (the operand
	 * pushed first is the left one) -- all in float, one rounding per operation.  At most 8 operands at once. */
	const int32_t* equation_offsets; /* [n_equations + 1] into the programs */
	const int32_t* program_op;       /* [n_program_ops] */
	const float* program_const;      /* [n_program_ops] */
	/* transitions: items in pointOrSlopeList() order.  items[i] = {kind, first_point, n_points, first_slope, n_slopes}:
	 * kind 0 a point (n_points 1, n_slopes 0), kind 1 a slope ratio, a run of points and the slopes between them. */
	const int32_t* transition_offsets; /* [n_transitions + 1] into the items */
	const int32_t* items;              /* [n_items][5] */
	const int32_t* point_type;         /* [n_points] 2 diphone, 3 triphone, 4 tetraphone */
	const float* point_value;          /* [n_points] */
	const float* point_free_time;      /* [n_points] milliseconds; read when point_time_eq is -1 */
	const int32_t* point_time_eq;      /* [n_points] the time equation, or -1 */
	const float* slopes;               /* [n_slopes] */
};
typedef struct gvtm_rules_model gvtm_rules_model;

/* One phone of an utterance.  tempo is postureData_.tempo AFTER applyRhythm(): feet and tone groups are the caller's. */
struct gvtm_posture {
	int32_t posture;    /* index into the model's postures */
	int32_t marked;     /* 0 or not */
	double tempo;
	double rule_tempo;  /* postureData_.ruleTempo: the rule that starts at this posture runs 1 / rule_tempo as long */
};
typedef struct gvtm_posture gvtm_posture;

/* EventList.h:85-103, one per rule application */
struct gvtm_rule_data {
	int32_t number;         /* the rule's index + 1 */
	int32_t first_posture, last_posture;
	int32_t start;          /* zeroRef_ at the rule's start, ms */
	double mark1, mark2, duration;
	double beat;            /* the rule's beat + start */
};
typedef struct gvtm_rule_data gvtm_rule_data;

typedef struct gvtm_rules gvtm_rules;

/* Checks the model, keeps a copy and, unless device is GVTM_DEVICE_NONE (host use only), uploads it; synchronous.
 * GVTM_ERR_INVALID_ARGUMENT, with the reason in gvtm_last_error(): a null argument or array, an index outside its table, a
 * rule without a parameter-profile transition, a special-profile transition that holds a slope ratio, a program that is
 * not a well-formed postfix expression or holds more than 8 operands at once, and -- where the reference throws when it
 * walks the transition -- a slope ratio that is empty or whose points are not its slopes plus one. */
int gvtm_rules_create(int device, const gvtm_rules_model* model, gvtm_rules** rules_out);
void gvtm_rules_destroy(gvtm_rules* rules);

/*
 * The rule for one utterance of n postures, on the host; needs no device.  Reproduced, not tidied: an event's time is
 * zeroRef + (int)time less its remainder by control_period, taken of the ABSOLUTE time, so with a rule start that is no
 * multiple of the period an event can fall before the start; insertEvent refuses a time below 0 or above the CURRENT
 * rule's (int)duration + control_period; a later value at the same (time, parameter) wins -- the parameter loop runs
 * before the special loop, rule k + 1's targets land on rule k's closing event, the last item of a transition (a slope
 * ratio's last point only if the ratio is the last item) is a phantom that inserts nothing; the equal-targets shortcut
 * compares the float targets widened to double; the marker events carry no value and still make an event of 32 empty
 * (+infinity) values; the intervals are checked against control_period + 1.  Every event has has_interp = 0, interp = 0.
 *
 * An utterance is refused with a status, its list empty and its rule count 0 (onsets are then not defined):
 *   0  ok
 *   1  no rule matches at some posture (the reference throws)
 *   2  "the time interval between two postures is too small" (the reference throws)
 *   3  where the reference is undefined: a rule symbol that is not finite (a rule_tempo of 0), an (int) of a value no int
 *      holds, a point time that is a NaN, a list that runs beyond INT_MAX ms
 *   4  a posture id outside the model, or fewer than two postures
 *   5  device only: the list does not fit behind the lists before it in out_capacity events, or one rule spans more
 *      than 4094 control periods (the kernels' window; the host has no such limit)
 * The first refusal in the reference's order of work decides.  (A list dropped for want of room in out_capacity had been
 * accepted by the rule: its rule data, rule count and onsets stand.)
 *
 *   events_out [capacity]          may be NULL (count only).  More events than capacity: GVTM_ERR_INVALID_ARGUMENT, with
 *                                  *n_events_out the count needed.
 *   rule_data_out [rule_capacity]  may be NULL; rows beyond rule_capacity are dropped, *n_rules_out counts them all
 *   onsets_out [n]                 may be NULL; postureData_[i].onset: 0 for the first posture, start + beat of its rule
 * Returns GVTM_OK also for a refused utterance; GVTM_ERR_INVALID_ARGUMENT for null rules, postures with n > 0, n_events_out
 * or status_out, or a control_period outside 1..4.
 */
int gvtm_rules_apply_host(const gvtm_rules* rules, int32_t control_period, const gvtm_posture* postures, size_t n,
		gvtm_event* events_out, size_t capacity, size_t* n_events_out, gvtm_rule_data* rule_data_out, size_t rule_capacity,
		size_t* n_rules_out, double* onsets_out, int32_t* status_out);
/* The count alone: events of the utterance (0 when refused; status_out may be NULL), or -1 on a bad call. */
int64_t gvtm_rules_event_count(const gvtm_rules* rules, int32_t control_period, const gvtm_posture* postures, size_t n,
		int32_t* status_out);

/*
 * The rule for a batch, everything resident in device memory.
 *   d_postures, d_posture_offsets [batch + 1] int64   utterance b owns the postures [off[b], off[b+1])
 *   d_events_out                  out, out_capacity events: the lists back to back in utterance order
 *   d_event_offsets_out [batch + 1] int64   out: exactly the d_event_offsets that gvtm_generate_tracks_device,
 *                                 gvtm_apply_intonation_device (as d_list_offsets) and the *_events_* entries take
 *   d_rule_data [batch][max_rules], d_rule_counts [batch] int32   out, either may be NULL: the rule data; rows beyond
 *                                 max_rules are dropped, the count covers them
 *   d_onsets                      out, may be NULL: one double per posture, laid out as d_postures
 *   d_status [batch] int32        out, may be NULL
 * Lists, offsets, rule data, onsets and statuses are bit for bit gvtm_rules_apply_host's, utterance by utterance.  Nothing
 * is written at or beyond out_capacity events and nothing for a refused utterance; a list that would end beyond
 * out_capacity is refused (5) and takes no room, so a shorter one behind it may still fit.  Enqueue-only: three kernels
 * on hip_stream (count, scan, write), no scratch.  GVTM_ERR_INVALID_ARGUMENT: null rules, with batch > 0 a null d_postures,
 * d_posture_offsets, d_events_out or d_event_offsets_out, a control_period outside 1..4; GVTM_ERR_NO_DEVICE: rules created
 * with GVTM_DEVICE_NONE; batch == 0 returns GVTM_OK.
 */
int gvtm_generate_events_device(const gvtm_rules* rules, int32_t control_period, const gvtm_posture* d_postures,
		const int64_t* d_posture_offsets, size_t batch, gvtm_event* d_events_out, size_t out_capacity,
		int64_t* d_event_offsets_out, gvtm_rule_data* d_rule_data, size_t max_rules, int32_t* d_rule_counts,
		double* d_onsets, int32_t* d_status, void* hip_stream);

/*
 * Postures in, audio out: gvtm_generate_events_device into an event buffer the plan owns (grown to events_capacity events:
 * the out_capacity above; gvtm_rules_event_count sizes it on the host), then gvtm_synthesize_events_device on those lists,
 * all enqueued on hip_stream.  Samples, counts, peaks, frame counts and drift states are bit for bit those of the two calls
 * made separately; a refused utterance has 0 frames.  config, max_frames and the audio arguments are
 * gvtm_synthesize_events_device's, for every plan that entry takes; the control period is config's.  The rules must live on
 * the plan's device.  The event buffer is one more buffer of the plan's that the one-stream ordering rule of that entry
 * covers.  Refused before any device work: what gvtm_synthesize_events_device and gvtm_generate_events_device refuse, and
 * rules on another device than the plan's (GVTM_ERR_INVALID_ARGUMENT).
 */
int gvtm_synthesize_postures_device(gvtm_plan* plan, const gvtm_rules* rules, const gvtm_track_config* config,
		const gvtm_posture* d_postures, const int64_t* d_posture_offsets, size_t events_capacity, size_t batch,
		size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts,
		float* d_maxabs, gvtm_drift_state* d_drift, int32_t* d_status, void* hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Rhythm and intonation points: the two steps of EventList that stand on either side of the rule above.
 * EventList::applyRhythm() (EventList.cpp:796-819) runs at the head of generateEventList() and turns feet into posture
 * tempi; EventList::applyIntonation() / addIntonationPoint() (:687-793, :903-927) runs behind it and places the
 * IntonationPoints by the rule data and the posture onsets.  With the entries below a batch goes from postures, feet and
 * tone groups to samples without leaving the device: bit for bit the reference's generateEventList(); applyIntonation();
 * generateOutput().  (The four structures of this section are declared in two steps, as those of the section above.)
 *
 * Rhythm, per foot in order: n = end - start + 1; tempo += (a * n + b) / div with the marked or the unmarked constants;
 * clamped to [min_tempo, max_tempo]; multiplied by global_tempo; then postures[j].tempo *= tempo for every posture of the
 * foot.  Postures in no foot keep their tempo.
 *
 * Points, per tone group and per foot of it in order: startTime and endTime are the onsets of feet[start_foot].start and
 * feet[end_foot].end; pretonicDelta = deltaTime < 1.0e-6 ? 0.0 : param[0] / deltaTime.  The posture of a foot is its first
 * vocoid, or `start` if it has none; its rule is the first row with first_posture <= p <= last_posture.  An unmarked
 * (pretonic) foot gets one point, semitone (onset[p] - startTime) * pretonicDelta + param[0] + r, slope
 * pretonic_base_slope, or with draws r = (draw[0] - 0.5) * param[2] and slope draw[1] * pretonic_slope_random_factor +
 * pretonic_base_slope_random.  A marked (tonic) foot gets two: semitone (param[1] + param[0], a float sum) + r, slope
 * tonic_base_slope (type 3: tonic_continuation_base_slope) + tonic_slope_offset, or with draws r = (draw[0] - 0.5) *
 * param[4] and + draw[1] * tonic_slope_random_factor; then, at the rule of feet[j].end searched from the rule of the first,
 * semitone param[1] + param[0] + param[3] (a float sum) with offset 0 and slope 0.  The offset is 0 for the first foot of
 * the utterance and time_offset for every foot behind it; it is not reset per group.  One closing point stands at the last
 * rule with the last group's param[1] + param[0] + param[3], offset 0, slope 0.  Every point goes through
 * addIntonationPoint: semitone and slope are multiplied by the float intonation_factor; time = max(beat + offset, 0);
 * minTime = (the time stored for the point before, or 0 for the first) + 2.0 * control_period; if time < minTime, offset +=
 * minTime - time; the time_ms stored is max(beat + offset, 0) once more, not minTime.  Floats widen to double where the C++
 * expression widens them; no FMA contraction; IEEE division.  An utterance without a tone group gets no points.
 *
 * An utterance is refused on its own, with 0 points, and by the prosody entry with 0 frames.  Its status, the first that
 * applies:
 *   0  ok
 *   1  a structure the reference could not have built: a foot outside the postures or with start > end, feet that are not
 *      strictly increasing and disjoint, a group outside the feet or with start_foot > end_foot, groups that are not
 *      increasing and disjoint, a type outside 0..5, a posture id outside the vocoid table
 *   2  an utterance the rules entry refused (any status but 0), no rule rows or more than max_rules, a posture in no row
 *   3  more than GVTM_MAX_INTONATION_POINTS points: feet in groups + marked feet in groups + 1
 *   4  a foot tempo (rhythm), a draw, a parameter or a resulting time, semitone or slope that is not finite
 *   5  device only: the points do not fit behind those before them in points_capacity
 * Rhythm knows 0, 1 and 4 only; a foot it refuses multiplies nothing, the largest status of an utterance's feet is the
 * utterance's, and the tempi of a refused utterance are not defined.
 */
struct gvtm_foot {
	int32_t start, end;   /* posture indices within the utterance, inclusive (feet_[i].start, .end) */
	int32_t marked;       /* 0 or not: a tonic foot */
	int32_t reserved_;
	double tempo;         /* Foot::tempo before rhythm: the parser's /f value, otherwise 1.0 */
};
typedef struct gvtm_foot gvtm_foot;

/* Only closed feet and closed groups are listed: the reference's loops stop at currentFoot_ and currentToneGroup_. */
struct gvtm_tone_group {
	int32_t start_foot, end_foot;  /* inclusive, into the utterance's feet */
	int32_t type;                  /* IntonationRhythm::ToneGroup 0..4 (3: continuation), 5: none */
	float param[5];                /* what intonationParameters(type) returned: notional pitch, pretonic pitch range, pretonic
	                                  perturbation range, tonic pitch range, tonic perturbation range.  Choosing the set
	                                  (fixed, first of the file, a random index) is the caller's. */
};
typedef struct gvtm_tone_group gvtm_tone_group;

/* Every number in the type the reference holds it in: intonation.txt, EventList::intonationFactor_, rhythm.txt,
 * EventList::globalTempo_. */
struct gvtm_prosody_config {
	float time_offset, pretonic_base_slope, pretonic_base_slope_random, pretonic_slope_random_factor;
	float tonic_base_slope, tonic_continuation_base_slope, tonic_slope_random_factor, tonic_slope_offset;
	float intonation_factor;
	float reserved_;
	double marked_a, marked_b, marked_div, unmarked_a, unmarked_b, unmarked_div, min_tempo, max_tempo;
	double global_tempo;
};
typedef struct gvtm_prosody_config gvtm_prosody_config;

typedef struct gvtm_prosody gvtm_prosody;

/* Checks and keeps the configuration and the table and, unless device is GVTM_DEVICE_NONE (host use only), uploads the
 * table; synchronous.  vocoid [n_postures]: is the posture a member of the category "vocoid" (control_model.compile_model
 * gives it beside the rules model).  GVTM_ERR_INVALID_ARGUMENT: a null argument -- a model without the category has no
 * table, which is the reference's UnavailableResourceException --, n_postures 0, a number that is not finite. */
int gvtm_prosody_create(int device, const gvtm_prosody_config* config, const uint8_t* vocoid, size_t n_postures,
		gvtm_prosody** prosody_out);
void gvtm_prosody_destroy(gvtm_prosody* prosody);

/* Rhythm for one utterance, on the host; needs no device.  postures_out [n] may be postures (in place).  Returns GVTM_OK
 * also for a refused utterance (*status_out 1 or 4). */
int gvtm_prosody_rhythm_host(const gvtm_prosody* prosody, const gvtm_posture* postures, size_t n, const gvtm_foot* feet,
		size_t n_feet, gvtm_posture* postures_out, int32_t* status_out);
/* The points the tables alone promise (0 without a group), or -1: a bad call, or a structure of status 1. */
int64_t gvtm_prosody_point_count(size_t n_postures, const gvtm_foot* feet, size_t n_feet, const gvtm_tone_group* groups,
		size_t n_groups);
/* The points of one utterance, on the host; needs no device.  postures: after rhythm, as the rules entry took them;
 * draws: two doubles in [0, 1) per foot, laid out as the feet -- [0] the semitone draw, [1] the slope draw, of a pretonic
 * and of a tonic foot alike -- or NULL: randomIntonation() is false; rule_data [n_rules], onsets [n] and rule_status: what
 * gvtm_rules_apply_host left.  points_out [capacity] may be NULL (count and status only).  Returns GVTM_OK also for a
 * refused utterance; GVTM_ERR_INVALID_ARGUMENT for a null argument, a control_period outside 1..4, more points than
 * capacity. */
int gvtm_prosody_points_host(const gvtm_prosody* prosody, int32_t control_period, const gvtm_posture* postures, size_t n,
		const gvtm_foot* feet, size_t n_feet, const gvtm_tone_group* groups, size_t n_groups, const double* draws,
		const gvtm_rule_data* rule_data, size_t n_rules, const double* onsets, int32_t rule_status,
		gvtm_intonation_point* points_out, size_t capacity, size_t* n_points_out, int32_t* status_out);

/* Rhythm for a batch, everything resident in device memory: postures and feet back to back, utterance b owning the
 * records between d_posture_offsets[b] and [b + 1] resp. d_foot_offsets[b] and [b + 1] (int64, [batch + 1]); n_postures
 * and n_feet are the records behind the two arrays (the tables' last entries, which the caller knows).  d_postures_out
 * [n_postures] may be d_postures (in place); otherwise the postures are copied first.  d_status [batch] may be NULL.
 * Bit for bit gvtm_prosody_rhythm_host's, utterance by utterance.  Enqueue-only: a copy, a clearing of the statuses and
 * one kernel, a lane per foot, on hip_stream.  GVTM_ERR_NO_DEVICE: an object created with GVTM_DEVICE_NONE. */
int gvtm_apply_rhythm_device(const gvtm_prosody* prosody, const gvtm_posture* d_postures, const int64_t* d_posture_offsets,
		size_t n_postures, const gvtm_foot* d_feet, const int64_t* d_foot_offsets, size_t n_feet, size_t batch,
		gvtm_posture* d_postures_out, int32_t* d_status, void* hip_stream);

/* The points for a batch.  d_postures (after rhythm), d_rule_data [batch][max_rules], d_rule_counts, d_onsets and d_status
 * are exactly what gvtm_generate_events_device took and left; d_status [batch] (may be NULL: every utterance counts as
 * accepted by the rule) is read and then overwritten with the statuses above.  d_groups, d_group_offsets as the feet;
 * d_draws two doubles per foot laid out as the feet, or NULL.  d_points_out [points_capacity] and d_point_offsets_out
 * [batch + 1] are exactly what gvtm_apply_intonation_device takes.  Points, offsets and statuses are bit for bit
 * gvtm_prosody_points_host's.  Nothing is written at or beyond points_capacity and nothing for a refused utterance; points
 * that would end beyond points_capacity are refused (5) and take no room.  Enqueue-only: three kernels on hip_stream. */
int gvtm_place_intonation_device(const gvtm_prosody* prosody, int32_t control_period, const gvtm_posture* d_postures,
		const int64_t* d_posture_offsets, const gvtm_foot* d_feet, const int64_t* d_foot_offsets,
		const gvtm_tone_group* d_groups, const int64_t* d_group_offsets, const double* d_draws, size_t batch,
		const gvtm_rule_data* d_rule_data, size_t max_rules, const int32_t* d_rule_counts, const double* d_onsets,
		gvtm_intonation_point* d_points_out, size_t points_capacity, int64_t* d_point_offsets_out, int32_t* d_status,
		void* hip_stream);

/* Postures, feet and tone groups in, audio out, on a plan with track configurations (gvtm_plan_set_voice_tracks):
 * gvtm_apply_rhythm_device, gvtm_generate_events_device, gvtm_place_intonation_device, gvtm_apply_intonation_device and
 * gvtm_synthesize_events_voices_device, all enqueued on hip_stream with buffers the plan owns in between: postures,
 * max_rules rule rows per utterance, onsets, events_capacity generated events, points_capacity points and events_capacity +
 * points_capacity merged events.  They are more buffers of the plan's that the one-stream ordering rule covers.  The
 * control period is the plan's.  The reference merges points only if macroIntonation_: an utterance whose voice has
 * macro_intonation 0 gets no points, its list is the generated one.  A refused utterance reaches the apply step with list
 * id -1 and so has 0 frames.  d_prosody_status [batch] (may be NULL) gets the statuses above, d_status [batch] (may be NULL)
 * gvtm_apply_intonation_device's.  Samples, counts, peaks, frame counts, drift states and statuses are bit for bit those
 * of the five calls made one by one.  Refused before any device work: a null plan, rules or prosody, a plan without track
 * configurations, a design-only plan, rules or a prosody object on another device than the plan's, and with batch > 0 a
 * null table, voice ids or audio buffer, a stride too short, max_rules 0. */
int gvtm_synthesize_prosody_device(gvtm_plan* plan, const gvtm_rules* rules, const gvtm_prosody* prosody,
		const gvtm_posture* d_postures, const int64_t* d_posture_offsets, size_t n_postures, const gvtm_foot* d_feet,
		const int64_t* d_foot_offsets, size_t n_feet, const gvtm_tone_group* d_groups, const int64_t* d_group_offsets,
		const double* d_draws, const int32_t* d_voice_ids, size_t max_rules, size_t points_capacity, size_t events_capacity,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts,
		float* d_maxabs, gvtm_drift_state* d_drift, int32_t* d_prosody_status, int32_t* d_status, void* hip_stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* GAMA_VTM_H_ */
