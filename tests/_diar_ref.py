"""An O(N) numpy restatement of the diarization ops in this project's own words: the oracle for inputs too long for a fixture, and for the
machines where only this repository exists.  tests/test_diarization.py holds it to the reference's outputs (tests/golden/diarization.npz)."""
import numpy as np


def out_len(L, K):
	return L + 2 * (K // 2) - K + 1


def sliding_max(x, K):
	"""Rows of x (C, L): out[c][i] = max of the -inf padded row over [i, i + K - 1] (padding K // 2 on both sides).  Block prefix / suffix maxima."""
	x = np.asarray(x, dtype = np.float32)
	C, L = x.shape
	Lo = out_len(L, K)
	nb = (Lo + K - 1 + K - 1) // K  # blocks of K that cover the Lo + K - 1 padded positions in use
	p = np.full((C, nb * K), -np.inf, dtype = np.float32)
	lo = K // 2
	take = min(L, nb * K - lo)
	p[:, lo:lo + take] = x[:, :take]
	blocks = p.reshape(C, nb, K)
	g = np.maximum.accumulate(blocks, axis = 2).reshape(C, -1)
	h = np.maximum.accumulate(blocks[:, :, ::-1], axis = 2)[:, :, ::-1].reshape(C, -1)
	return np.maximum(h[:, :Lo], g[:, K - 1:K - 1 + Lo])


def sliding_min(x, K):
	return -sliding_max(-np.asarray(x, dtype = np.float32), K)


def kth_value(x, k):
	"""k-th smallest per row, k 1-based."""
	return np.partition(np.asarray(x), k - 1, axis = -1)[..., k - 1]


def sign_prefix_sum(d):
	return np.cumsum(np.sign(d[0].astype(np.float64) - d[1].astype(np.float64)).astype(np.int64)).astype(np.int32)


def box_sign(s, K):
	"""sign of the zero-padded box sum of the integer sequence s over window K, padding K // 2."""
	L = len(s)
	Lo = out_len(L, K)
	P = np.concatenate(([0], np.cumsum(s.astype(np.int64))))
	i = np.arange(Lo)
	lo, hi = np.clip(i - K // 2, 0, L), np.clip(i - K // 2 + K, 0, L)
	return np.sign(P[hi] - P[lo]).astype(np.int64)


def select_speaker(signal, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker, silence_absolute_threshold = 0.2,
                   silence_relative_threshold = 0.5, eps = 1e-9, normalization_percentile = 0.9):
	"""-> (speaker_id (L,) float32, mask (3, L) bool)."""
	a = np.abs(np.asarray(signal, dtype = np.float32))
	smoothed = sliding_max(a, kernel_size_smooth_signal)
	eroded = sliding_min(sliding_max(a, kernel_size_smooth_silence), kernel_size_smooth_silence)
	k = int(normalization_percentile * smoothed.shape[1])
	assert k >= 1
	kth = kth_value(smoothed, k).astype(np.float32)
	f = np.float32
	silence = (eroded < f(silence_absolute_threshold)) | ((eroded / (f(eps) + kth)[:, None]).astype(np.float32) < f(silence_relative_threshold))
	s = (smoothed[0] > smoothed[1]).astype(np.int64) - (smoothed[0] < smoothed[1]).astype(np.int64)
	b = box_sign(s, kernel_size_smooth_speaker)
	left, right = np.concatenate(([0], b[:-1])), np.concatenate((b[1:], [0]))
	b = np.where((b == 0) & (left != 0) & (left + right == 0), 1, b)
	L = min(eroded.shape[1], len(b))
	silence, b = silence[:, :L], b[:L]
	both = silence.all(axis = 0)
	speaker_id = np.where(both | (b == 0), 0.0, np.where(b > 0, 1.0, 2.0)).astype(np.float32)
	return speaker_id, np.stack([both, ~silence[0] & (b == 1), ~silence[1] & (b == -1)])


def speaker_mask(transcript, num_speakers, duration, sample_rate):
	"""(1 + num_speakers, int(duration * sample_rate)) bool: row s covers the sample positions of speaker s's segments, row 0 the overlap."""
	rows = np.zeros((1 + num_speakers, int(duration * sample_rate)), dtype = bool)
	for segment in transcript:
		first, stop = int(segment['begin'] * sample_rate), int(segment['end'] * sample_rate)
		rows[segment['speaker'], first:stop] = True
	rows[0] = np.logical_and(rows[1], rows[2])
	return rows


def speaker_error_counts(ref_mask, hyp_mask, perm):
	r1, r2, h1, h2 = ref_mask[1], ref_mask[2], hyp_mask[perm[1]], hyp_mask[perm[2]]
	mismatch, kept = (r1 != h1) | (r2 != h2), r1 != r2
	return [int(v.sum()) for v in (mismatch & kept, mismatch, (h1 & r2 & ~r1) | (h2 & r1 & ~r2), (h1 | h2) & ~r1 & ~r2, ~h1 & ~h2 & (r1 | r2), kept, r1 | r2)]


def speaker_error(ref, hyp, sample_rate = 8000, hyp_speaker_mapping = None, ignore_silence_and_overlapped_speech = True):
	duration = max(t['end'] for tr in (hyp, ref) for t in tr)
	rm, hm = speaker_mask(ref, 2, duration, sample_rate), speaker_mask(hyp, 2, duration, sample_rate)
	vals = []
	for perm in ([[0, 1, 2], [0, 2, 1]] if hyp_speaker_mapping is None else hyp_speaker_mapping):
		c = speaker_error_counts(rm, hm, perm)
		num, den = (c[0], c[5]) if ignore_silence_and_overlapped_speech else (c[1], rm.shape[1])
		with np.errstate(invalid = 'ignore', divide = 'ignore'):
			vals.append((float(np.float32(num) / np.float32(den)), list(perm)))
	return min(vals)
