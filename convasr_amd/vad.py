"""Speech-activity detection on the GPU and the cutting of a long recording into utterance-sized segments (reference: vad.py, whose goals are
"augmenting decoding, batching, cuts for model-less dataset creation" and whose postprocess_cut / postprocess_batching are empty stubs).

The reference's detector is webrtcvad, a C library this project does not have.  The detector here is this project's own, defined exactly in
include/convasr_hip.h and unpinned against webrtcvad: the peak of every frame (csrc/vad.hip, the one pass over the samples), a level per
channel (a percentile of the peaks), select_speaker's silence test per frame, three smoothing steps on whole frames (fill short gaps, drop
short bursts, pad), and the speech runs cut at their quietest frames into pieces of at most max_duration.  Every step is an O(N) or O(frames)
kernel and every result exact.  Python-level argument errors raise ValueError; a CPU signal raises ConvasrHipError before any launch: there
is no host path."""
import torch

from . import _lib, ops
from .transcript_generators import Segment, Transcript

# aggressiveness -> (absolute threshold, threshold relative to the channel's level); 3 is the pair of the reference's `ref` diarization command
THRESHOLDS = {0: (0.005, 0.02), 1: (0.01, 0.05), 2: (0.02, 0.1), 3: (0.05, 0.2)}
PERCENTILE, EPS = 0.9, 1e-9
MIN_GAP, MIN_SPEECH, PAD = 1.0, 0.5, 0.2  # seconds; the first two are the numbers in the comments of the reference's postprocess_cut
MAX_CHANNELS, MAX_SAMPLES, MAX_FRAME = _lib.VAD_MAX_CHANNELS, _lib.VAD_MAX_LEN, _lib.VAD_MAX_FRAME


def frames_of(seconds, window_size):
	"""A duration as whole frames: int(round(seconds / window_size))."""
	return int(round(seconds / window_size))


def settings(sample_rate, window_size, aggressiveness, window_size_dilate = None, abs_thr = None, rel_thr = None, percentile = PERCENTILE, eps = EPS, min_gap = MIN_GAP,
             min_speech = MIN_SPEECH, pad = PAD, gap_frames = None, speech_frames = None, pad_frames = None):
	"""The presets with their overrides resolved: dict(F, abs_thr, rel_thr, percentile, eps, G, S, P).  F = int(window_size * sample_rate), as in
	the reference; G, S, P = frames_of(min_gap / min_speech / pad) unless given as frame counts; window_size_dilate sets
	P = int(window_size_dilate / window_size) // 2 (the half-width of the dilation the reference left commented out)."""
	if abs_thr is None or rel_thr is None:
		if aggressiveness not in THRESHOLDS:
			raise ValueError(f'vad: aggressiveness = {aggressiveness!r}, one of {sorted(THRESHOLDS)} expected')
		abs_thr, rel_thr = (THRESHOLDS[aggressiveness][0] if abs_thr is None else abs_thr), (THRESHOLDS[aggressiveness][1] if rel_thr is None else rel_thr)
	if not window_size > 0 or not sample_rate > 0:
		raise ValueError(f'vad: window_size = {window_size} s at {sample_rate} Hz, positive values expected')
	F = int(window_size * sample_rate)
	if not 1 <= F <= MAX_FRAME:
		raise ValueError(f'vad: a frame of int({window_size} * {sample_rate}) = {F} samples, 1 to {MAX_FRAME} expected')
	G = frames_of(min_gap, window_size) if gap_frames is None else int(gap_frames)
	S = frames_of(min_speech, window_size) if speech_frames is None else int(speech_frames)
	P = (int(window_size_dilate / window_size) // 2 if window_size_dilate is not None else frames_of(pad, window_size)) if pad_frames is None else int(pad_frames)
	if min(G, S, P) < 0:
		raise ValueError(f'vad: negative smoothing length (gap {G}, speech {S}, pad {P} frames)')
	if not 0.0 <= percentile <= 1.0:
		raise ValueError(f'vad: percentile = {percentile}, 0 to 1 expected')
	return dict(F = F, abs_thr = float(abs_thr), rel_thr = float(rel_thr), percentile = float(percentile), eps = float(eps), G = G, S = S, P = P)


def _check_signal(name, signal):
	if not torch.is_tensor(signal) or signal.ndim != 2:
		raise ValueError(f'{name}: signal must be a (C, N) tensor, got {tuple(signal.shape) if torch.is_tensor(signal) else type(signal)}')
	if signal.dtype not in (torch.float32, torch.int16):
		raise ValueError(f'{name}: signal must be float32 or int16, got {signal.dtype}')
	C, N = signal.shape
	if not 1 <= C <= MAX_CHANNELS:
		raise ValueError(f'{name}: {C} channels, 1 to {MAX_CHANNELS} expected')
	if not 1 <= N <= MAX_SAMPLES:
		raise ValueError(f'{name}: N = {N} samples per channel, 1 to {MAX_SAMPLES} (2^28) expected')
	_lib.require_cuda(signal)
	return C, N


def _frames(name, signal, cfg):
	C, N = _check_signal(name, signal)
	peaks = ops.frame_peaks(signal, cfg['F'])
	n_full = N // cfg['F']
	k = max(1, int(cfg['percentile'] * n_full))
	_, mask = ops.vad_frames(peaks, n_full, cfg['abs_thr'], cfg['rel_thr'], cfg['eps'], k, cfg['G'], cfg['S'], cfg['P'])
	return mask, peaks, N


def detect_speech_frames(signal, sample_rate, window_size, aggressiveness, window_size_dilate = None, **overrides):
	"""The smoothed speech mask per frame and the frame peaks: ((C, nF) bool, (C, nF) float32), nF = ceil(N / F).  overrides: see settings."""
	mask, peaks, _ = _frames('detect_speech_frames', signal, settings(sample_rate, window_size, aggressiveness, window_size_dilate, **overrides))
	return mask, peaks


def detect_speech(signal, sample_rate, window_size, aggressiveness, window_size_dilate = None, **overrides):
	"""vad.py:12-25 with this project's detector.  signal: (C, N) float32 or int16 on the device.  Returns a (C, N) bool mask on the signal's
	device: the smoothed frame mask, every frame repeated F = int(window_size * sample_rate) times and cut to N."""
	cfg = settings(sample_rate, window_size, aggressiveness, window_size_dilate, **overrides)
	mask, _, N = _frames('detect_speech', signal, cfg)
	return mask.repeat_interleave(cfg['F'], dim = -1)[:, :N]


def segments(signal, sample_rate, window_size = 0.02, aggressiveness = 2, window_size_dilate = None, max_duration = 15.0, audio_path = None, **overrides):
	"""The speech of a recording as a Transcript of Segment(begin, end, channel, first, count[, audio_path]), by channel and then time: the runs
	of the smoothed mask, those longer than max_duration (frames_of(max_duration) frames; None or 0: no cutting) cut at their quietest frames.
	first / count are the segment's samples, begin = first / sample_rate and end = (first + count) / sample_rate; ops.gather_segments takes the
	integers, never int(begin * sample_rate)."""
	cfg = settings(sample_rate, window_size, aggressiveness, window_size_dilate, **overrides)
	M = frames_of(max_duration, window_size) if max_duration else 0
	if M == 1 or M < 0:
		raise ValueError(f'vad.segments: max_duration = {max_duration} s is {M} frame(s) of {window_size} s; at least 2, or 0 for no cutting, expected')
	mask, peaks, N = _frames('vad.segments', signal, cfg)
	channel, first, count = (t.tolist() for t in torch.stack(ops.vad_segments(mask, peaks, cfg['F'], N, M)).cpu())
	transcript = Transcript()
	for c, a, n in zip(channel, first, count):
		segment = Segment() if audio_path is None else Segment(audio_path = audio_path)
		segment.update(begin = a / sample_rate, end = (a + n) / sample_rate, channel = c, first = a, count = n)
		transcript.append(segment)
	return transcript


def segment_samples(begin, end, sample_rate, N):
	"""(first, count) of the samples AudioTextDataset takes for a transcript segment in its batched_transcript mode (datasets.py:261-262): from
	int(begin * sample_rate) up to and including int(end * sample_rate), inside the N samples of the recording."""
	first = int(begin * sample_rate)
	return first, min(N, 1 + int(end * sample_rate)) - first


def upsample(speech, log_probs):
	"""vad.py:45-48: a (C, n) speech mask at the time resolution of log_probs (..., T) -- nearest-neighbour interpolation to T positions, on
	log_probs's device, as bool.  Plain torch."""
	as_float = speech.to(device = log_probs.device, dtype = torch.float32).unsqueeze(1)
	return torch.nn.functional.interpolate(as_float, size = (log_probs.shape[-1], )).squeeze(1).round().to(torch.bool)
