"""Two-channel diarization (reference: diarization.py): select_speaker, a channel-energy diarizer with a primitive VAD for call recordings
with one speaker per channel and cross-talk; speaker_error, which scores a diarization against another; diarize, which turns a recording
into speaker segments (the body of the reference's `ref` command, diarization.py:116-122).

The reference writes select_speaker as max_pool1d / avg_pool1d with windows of up to 4,096 samples at stride 1 and a kthvalue over the whole
recording; here every step is an O(N) kernel (csrc/diar.hip) and the results are the reference's bit for bit.  Out of scope: the webrtcvad
and pyannote models, `der`, the file walking of ref / hyp / eval and their json / rttm / html writers."""
import torch

from . import _lib, metrics, models, ops
from .transcript_generators import Segment, Transcript

speaker_missing = 0
default_speaker_names = '_ABCDEFGHIJKLMNOPQRSTUVWXYZ'  # index = speaker number; speaker 0 (nobody) has the placeholder name

MAX_KERNEL_SIZE = _lib.DIAR_MAX_KERNEL
MAX_SAMPLES = _lib.DIAR_MAX_LEN


def convert_speaker_id(speaker_id, to_bipole = False, from_bipole = False):
	"""Speaker numbers between the categorical coding {0: nobody, 1, 2} and the bipole coding {0: nobody, +1: speaker 1, -1: speaker 2}, as
	the reference's function of this name: to_bipole maps 1 -> +1 and 2 -> -1, from_bipole maps +1 -> 1 and -1 -> 2; 0 stays 0.  The result
	is a tensor of the input's dtype.  Exactly one of the two flags must be set."""
	if bool(to_bipole) == bool(from_bipole):
		raise ValueError('convert_speaker_id: set exactly one of to_bipole and from_bipole')
	sources, targets = ((1, 2), (1, -1)) if to_bipole else ((1, -1), (1, 2))
	out = torch.zeros_like(speaker_id)
	for source, target in zip(sources, targets):
		out = torch.where(speaker_id == source, torch.full_like(speaker_id, target), out)
	return out


def _out_len(L, K):
	return L + 2 * (K // 2) - K + 1


def select_speaker(signal, kernel_size_smooth_silence: int, kernel_size_smooth_signal: int, kernel_size_smooth_speaker: int, silence_absolute_threshold: float = 0.2,
                   silence_relative_threshold: float = 0.5, eps: float = 1e-9, normalization_percentile = 0.9):
	"""diarization.py:58-99.  signal: (2, N) float32 tensor on the device, finite samples (assumed, not checked).  Returns
	(speaker_id_categorical (L,) float32 in {0, 1, 2}, mask (3, L) bool: row 0 both channels silent, rows 1 / 2 speaker 1 / 2 talking), on the
	signal's device.  L = N for odd kernel sizes and up to N + 2 for even ones, as in the reference.

	Envelope: float32, shape (2, N) with 1 <= N <= 2^28, kernel sizes in [1, 16384], int(normalization_percentile * L1) >= 1 (L1 = the length
	of the smoothed signal): outside it ValueError.  A CPU tensor raises ConvasrHipError before any launch; there is no host path."""
	if not torch.is_tensor(signal) or signal.ndim != 2 or signal.shape[0] != 2:
		raise ValueError(f'select_speaker: signal must be a (2, N) tensor, got {tuple(signal.shape) if torch.is_tensor(signal) else type(signal)}')
	if signal.dtype != torch.float32:
		raise ValueError(f'select_speaker: signal must be float32, got {signal.dtype}')
	N = signal.shape[1]
	if not 1 <= N <= MAX_SAMPLES:
		raise ValueError(f'select_speaker: N = {N} samples per channel, 1 to {MAX_SAMPLES} (2^28) expected')
	ks = dict(kernel_size_smooth_silence = kernel_size_smooth_silence, kernel_size_smooth_signal = kernel_size_smooth_signal, kernel_size_smooth_speaker = kernel_size_smooth_speaker)
	for name, K in ks.items():
		if int(K) != K or not 1 <= K <= MAX_KERNEL_SIZE:
			raise ValueError(f'select_speaker: {name} = {K}, an integer from 1 to {MAX_KERNEL_SIZE} expected')
	L1 = _out_len(N, int(kernel_size_smooth_signal))
	k = int(normalization_percentile * L1)
	if not 1 <= k <= L1:
		raise ValueError(f'select_speaker: int(normalization_percentile * {L1}) = {k}, a rank from 1 to {L1} expected')
	_lib.require_cuda(signal)
	return ops.select_speaker(signal.contiguous(), kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker, silence_absolute_threshold,
	                          silence_relative_threshold, eps, k)


def segments_from_runs(speaker, starts, lengths, values, sample_rate, audio_path = None):
	"""The runs of one speaker's mask row (host lists: first sample, samples, value of each run) -> one Segment per run of ones, in seconds:
	keys [audio_path,] begin, end, speaker, speaker_name."""
	segments = []
	for first_sample, n_samples, talking in zip(starts, lengths, values):
		if talking != 1:
			continue
		segment = Segment() if audio_path is None else Segment(audio_path = audio_path)
		segment['begin'] = float(first_sample) / sample_rate
		segment['end'] = (float(first_sample) + float(n_samples)) / sample_rate
		segment['speaker'] = speaker
		segment['speaker_name'] = default_speaker_names[speaker]
		segments.append(segment)
	return segments


def diarize(signal, sample_rate, audio_path = None, kernel_size_smooth_silence = 4096, kernel_size_smooth_signal = 128, kernel_size_smooth_speaker = 4096,
            silence_absolute_threshold = 0.05, silence_relative_threshold = 0.2, **select_speaker_kwargs):
	"""The reference's `ref` command for one recording (diarization.py:116-122), with its parameter values as defaults: select_speaker, then the
	runs of the mask rows of speakers 1 and 2 as a Transcript of Segment(begin, end, speaker, speaker_name[, audio_path]) in seconds, ordered by
	speaker, then time."""
	_, mask = select_speaker(signal, kernel_size_smooth_silence = kernel_size_smooth_silence, kernel_size_smooth_signal = kernel_size_smooth_signal,
	                         kernel_size_smooth_speaker = kernel_size_smooth_speaker, silence_absolute_threshold = silence_absolute_threshold,
	                         silence_relative_threshold = silence_relative_threshold, **select_speaker_kwargs)
	transcript = Transcript()
	for speaker in range(1, len(mask)):
		starts, lengths, values = [t.cpu().tolist() for t in models.rle1d(mask[speaker])]
		transcript.extend(segments_from_runs(speaker, starts, lengths, values, sample_rate, audio_path))
	return transcript


def speaker_mask(transcript, num_speakers, duration, sample_rate):
	"""Host mask of who talks when: (1 + num_speakers, int(duration * sample_rate)) bool.  Row s is True over the positions
	[int(begin * sample_rate), int(end * sample_rate)) of every segment of speaker s; row 0 is True where speakers 1 and 2 talk at once."""
	positions = int(duration * sample_rate)
	rows = torch.zeros(1 + num_speakers, positions, dtype = torch.bool)
	for segment in transcript:
		first, stop = int(segment['begin'] * sample_rate), int(segment['end'] * sample_rate)
		rows[segment['speaker']][first:stop] = True
	rows[0] = torch.logical_and(rows[1], rows[2])
	return rows


def compute_duration(ref, hyp):
	"""The latest end of any segment of the two transcripts, in seconds (what the reference scores a pair of transcripts over)."""
	ends = [segment['end'] for segment in hyp] + [segment['end'] for segment in ref]
	return max(ends)


def speaker_error(ref, hyp, num_speakers, sample_rate = 8000, hyp_speaker_mapping = None, ignore_silence_and_overlapped_speech = True, device = None):
	"""diarization.py:175-201.  ref, hyp: host transcripts (lists of dicts with begin, end, speaker).  Returns (err, mapping): over the
	mappings of the hypothesis's speakers ([0, 1, 2] and [0, 2, 1], or hyp_speaker_mapping), the smallest share of positions where a speaker
	row differs -- counted where exactly one reference speaker talks, or everywhere with ignore_silence_and_overlapped_speech = False --
	ties broken as Python compares (err, mapping) tuples.  The masks are built on the host as in the reference; the counts of every mapping come
	from one pass on the device (ops.speaker_error_counts).  err is the float32 quotient count / positions, nan when no position is kept."""
	if num_speakers != 2:
		raise ValueError(f'speaker_error: num_speakers = {num_speakers}, only 2 is implemented (as in the reference)')
	perms = [[0, 1, 2], [0, 2, 1]] if hyp_speaker_mapping is None else [list(p) for p in hyp_speaker_mapping]
	if not 1 <= len(perms) <= _lib.SPEAKER_MAX_PERMS:
		raise ValueError(f'speaker_error: {len(perms)} mappings, 1 to {_lib.SPEAKER_MAX_PERMS} expected')
	duration = compute_duration(ref, hyp)
	ref_mask, hyp_mask = speaker_mask(ref, num_speakers, duration, sample_rate), speaker_mask(hyp, num_speakers, duration, sample_rate)
	if ref_mask.shape[1] < 1:
		raise ValueError(f'speaker_error: a duration of {duration} s at {sample_rate} Hz leaves no position to score')
	device = metrics._device(device)
	counts = ops.speaker_error_counts(ref_mask.to(device), hyp_mask.to(device), perms).cpu()
	n = ref_mask.shape[1]
	vals = []
	for perm, c in zip(perms, counts.tolist()):
		mismatch, kept = (c[0], c[5]) if ignore_silence_and_overlapped_speech else (c[1], n)
		err = float(torch.tensor(float(mismatch), dtype = torch.float32) / torch.tensor(float(kept), dtype = torch.float32))
		vals.append((err, perm))
	return min(vals)
