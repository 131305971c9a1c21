"""What the track-generation tests share beyond event_lists.py's lists: the product's configuration record from the ten
numbers of a captured call, lists every model can sing, and drift-generator states."""
import numpy as np

import gama_tts_amd as g
import event_lists
import oracle


def product_config(cfg):
    """cfg: the ten numbers of oracle.track_config -- control period, macro, micro, drift, smooth, initial pitch, mean
    pitch, drift deviation / sample rate / cutoff."""
    c = g.TrackConfig()
    c.control_period_ms, c.macro_intonation, c.micro_intonation, c.intonation_drift, c.smooth_intonation = (int(x) for x in cfg[:5])
    c.initial_pitch, c.mean_pitch, c.drift_deviation, c.drift_sample_rate, c.drift_lowpass_cutoff = (float(x) for x in cfg[5:10])
    return c


def singable_event_table(seed, n_events):
    """event_lists.random_event_table with macro-intonation polynomials that keep the pitch inside the model's range
    (the generator's cubic and quadratic terms reach hundreds of semitones after half a second: fine for comparing FRAMES,
    but the oscillator then steps past its 512-entry wavetable, in the reference as here, and what comes out is whatever
    lies behind the table)."""
    return make_singable(event_lists.random_event_table(seed, n_events=n_events))


def make_singable(t):
    t[:, 2] = 0.0
    t[:, 3] = 0.0
    t[:, 4] *= 0.1
    t[:, 5] *= 0.5
    return t


def fresh_drift(batch):
    return np.tile(np.array(oracle.FRESH_DRIFT, dtype=np.float64), (batch, 1))


def used_drift(batch, seed=5):
    d = fresh_drift(batch)
    d[:, 0] = 0.1 + 0.8 * np.random.default_rng(seed).random(batch)  # generators that have run before
    return d
