"""numpy restatement of the speech-activity detector, the segment cutting and the gather that include/convasr_hip.h defines (convasr_frame_peak,
convasr_vad_frames, convasr_vad_segments_*, convasr_gather_segments) and of the host rules of convasr_amd/vad.py.  Written as loops over
frames and runs, one channel at a time; it shares no code with the package.  Checked on the CPU by tests/test_vad_ref.py."""
import math

import numpy as np

THRESHOLDS = {0: (0.005, 0.02), 1: (0.01, 0.05), 2: (0.02, 0.1), 3: (0.05, 0.2)}


def n_frames(N, F):
	return -(-N // F), N // F  # (all frames, whole frames)


def frame_peaks(signal, F):
	"""signal (C, N) float32 or int16 -> (C, nF) float32."""
	C, N = signal.shape
	nF, _ = n_frames(N, F)
	out = np.zeros((C, nF), np.float32)
	for c in range(C):
		for f in range(nF):
			chunk = signal[c, f * F:min((f + 1) * F, N)]
			if signal.dtype == np.int16:
				out[c, f] = np.float32(np.abs(chunk.astype(np.int32)).max()) / np.float32(32767)
			else:
				out[c, f] = np.abs(chunk).max()
	return out


def rank(percentile, nfull):
	return max(1, int(percentile * nfull))


def level(peaks, nfull, k):
	"""The k-th smallest (1-based) of the whole frames' peaks, per channel."""
	return np.array([np.sort(row[:nfull])[k - 1] for row in peaks], np.float32)


def raw_mask(peaks, nfull, lev, abs_thr, rel_thr, eps):
	C, nF = peaks.shape
	abs_thr, rel_thr, eps = np.float32(abs_thr), np.float32(rel_thr), np.float32(eps)
	out = np.zeros((C, nF), bool)
	with np.errstate(divide = 'ignore', invalid = 'ignore'):
		for c in range(C):
			denom = np.float32(eps + np.float32(lev[c]))
			for f in range(nfull):
				p = np.float32(peaks[c, f])
				out[c, f] = not (p < abs_thr or np.float32(p / denom) < rel_thr)
	return out


def runs_of(row, value = True):
	"""[a, b) of every maximal run of `value` in a 1-D bool array."""
	out, a = [], None
	for i, v in enumerate(list(row) + [not value]):
		if v == value and a is None:
			a = i
		elif v != value and a is not None:
			out.append((a, i))
			a = None
	return out


def smooth_row(row, G, S, P):
	n = len(row)
	step1 = np.array(row, bool)
	for a, b in runs_of(row, False):
		if a > 0 and b < n and b - a < G:
			step1[a:b] = True
	step2 = step1.copy()
	for a, b in runs_of(step1, True):
		if b - a < S:
			step2[a:b] = False
	step3 = step2.copy()
	for a, b in runs_of(step2, True):
		step3[max(0, a - P):min(n, b + P)] = True
	return step3


def smooth(raw, G, S, P):
	return np.stack([smooth_row(row, G, S, P) for row in raw])


def cut_run(a, b, peaks_row, M):
	"""The pieces [a', b') of the run [a, b): at most M frames each (M = 0: the run itself)."""
	out = []
	if M >= 2:
		while b - a > M:
			lo = a + -(-M // 2)
			j = lo
			for i in range(lo, a + M):
				if peaks_row[i] < peaks_row[j]:
					j = i
			out.append((a, j))
			a = j
	out.append((a, b))
	return out


def segment_frames(mask, peaks, M):
	"""[(channel, a, b)] in frames, by channel and then time."""
	return [(c, a2, b2) for c in range(mask.shape[0]) for a, b in runs_of(mask[c], True) for a2, b2 in cut_run(a, b, peaks[c], M)]


def segments(mask, peaks, F, N, M):
	"""(channel, first, count) lists in samples."""
	out = [(c, a * F, min(b * F, N) - a * F) for c, a, b in segment_frames(mask, peaks, M)]
	return [s[0] for s in out], [s[1] for s in out], [s[2] for s in out]


def seconds(first, count, sample_rate):
	return first / sample_rate, (first + count) / sample_rate


def gather(signal, channel, first, count, multiple = 128):
	"""(x (B, Tpad) float32, xlen (B,) float32)."""
	Tpad = int(math.ceil(max(count) / multiple)) * multiple
	x = np.zeros((len(channel), Tpad), np.float32)
	for b, (c, a, n) in enumerate(zip(channel, first, count)):
		piece = signal[c, a:a + n]
		assert a >= 0 and n >= 1 and len(piece) == n
		x[b, :n] = piece.astype(np.float32) / np.float32(32767) if signal.dtype == np.int16 else piece
	return x, np.array([n / Tpad for n in count], np.float32)


def frames_of(seconds_, window_size):
	return int(round(seconds_ / window_size))


def settings(sample_rate, window_size, aggressiveness, window_size_dilate = None):
	abs_thr, rel_thr = THRESHOLDS[aggressiveness]
	P = int(window_size_dilate / window_size) // 2 if window_size_dilate is not None else frames_of(0.2, window_size)
	return dict(F = int(window_size * sample_rate), abs_thr = abs_thr, rel_thr = rel_thr, percentile = 0.9, eps = 1e-9, G = frames_of(1.0, window_size), S = frames_of(0.5, window_size), P = P)


def detect_frames(signal, cfg):
	"""(peaks, raw, mask) of a signal under settings `cfg`."""
	C, N = signal.shape
	nF, nfull = n_frames(N, cfg['F'])
	peaks = frame_peaks(signal, cfg['F'])
	if nfull == 0:
		return peaks, np.zeros((C, nF), bool), np.zeros((C, nF), bool)
	raw = raw_mask(peaks, nfull, level(peaks, nfull, rank(cfg['percentile'], nfull)), cfg['abs_thr'], cfg['rel_thr'], cfg['eps'])
	return peaks, raw, smooth(raw, cfg['G'], cfg['S'], cfg['P'])


def detect_speech(signal, cfg):
	_, _, mask = detect_frames(signal, cfg)
	return np.repeat(mask, cfg['F'], axis = 1)[:, :signal.shape[1]]


def segment_samples(begin, end, sample_rate, N):
	first = int(begin * sample_rate)
	return first, min(N, 1 + int(end * sample_rate)) - first


def bursts(C, N, dtype, seed, sample_rate = 8000):
	"""A test recording: bursts of noise of varying amplitude between stretches of zeros and of faint noise, the channels unlike each other."""
	rng = np.random.default_rng(seed)
	x = np.zeros((C, N), np.float32)
	for c in range(C):
		at = 0
		while at < N:
			n = int(rng.integers(1, max(2, sample_rate)))
			kind = int(rng.integers(0, 3))
			if kind == 1:
				x[c, at:at + n] = rng.uniform(-1, 1, min(n, N - at)) * 0.003
			elif kind == 2:
				x[c, at:at + n] = rng.uniform(-1, 1, min(n, N - at)) * rng.uniform(0.05, 1.0)
			at += n
	if dtype == np.int16:
		pcm = np.round(x * 32767).astype(np.int16)
		pcm[0, N // 2] = -32768
		return pcm
	return x
