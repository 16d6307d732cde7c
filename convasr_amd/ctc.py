"""Host mirror of the reference's ctc.py: forced alignment on the GPU; and this package's own keyword search (`search`)."""
import torch

from . import ops


def alignment(log_probs, targets, input_lengths, target_lengths, blank: int = 0, pack_backpointers: bool = False):
	"""ctc.alignment (ctc.py:7-75): log_probs (T, B, C) like the reference, or this package's channels-last (B, C, T) tensor
	via `alignment_bct`.  Returns (B, S_max) int64: the last frame of the best path inside every label's state.
	pack_backpointers is accepted for signature parity; the kernel always packs (2 bits per state)."""
	lp = log_probs.float().permute(1, 0, 2).contiguous()
	return ops.ctc_alignment(lp, targets, input_lengths, target_lengths, blank)


def alignment_bct(log_probs_bct, targets, input_lengths, target_lengths, blank: int = 0):
	"""Same for the model's own output layout: logical (B, C, T) whose memory is (B, T, C)."""
	assert ops.is_cl(log_probs_bct)
	return ops.ctc_alignment(log_probs_bct.permute(0, 2, 1).float().contiguous(), targets, input_lengths, target_lengths, blank)


def alignment_long(log_probs, targets, input_lengths, target_lengths, blank: int = 0, pack_backpointers: bool = False, chunk_frames: int = 0):
	"""`alignment` for whole recordings: up to 131,071 labels over up to 2^20 frames (an hour of speech and more) on many compute units,
	valid at every target length and bit-equal to `alignment` where that takes the targets.  chunk_frames: see ops.ctc_alignment_long."""
	lp = log_probs.float().permute(1, 0, 2).contiguous()
	return ops.ctc_alignment_long(lp, targets, input_lengths, target_lengths, blank, chunk_frames = chunk_frames)


def alignment_long_bct(log_probs_bct, targets, input_lengths, target_lengths, blank: int = 0, chunk_frames: int = 0):
	"""Same for the model's own output layout: logical (B, C, T) whose memory is (B, T, C)."""
	assert ops.is_cl(log_probs_bct)
	return ops.ctc_alignment_long(log_probs_bct.permute(0, 2, 1).float().contiguous(), targets, input_lengths, target_lengths, blank, chunk_frames = chunk_frames)


def search(log_probs, tokens, token_lengths, blank, thresholds, lengths = None, min_gap: int = 10, max_hits: int = 16, dense: bool = False):
	"""Where each of K phrases is said in every utterance, and how sure the model is (this package's own detector; the reference has none, and it is
	unpinned against any outside keyword spotter): log_probs (T, B, C) as `alignment` takes them, log-probs or logits; tokens (K, L_max) and
	token_lengths (K,) the phrases' labels; thresholds a float or (K,) values; lengths (B,) frames or None; min_gap in frames.  Returns
	ops.ctc_keyword_search's namespace: count (B, K), score / begin / end (B, K, H), dense_score / dense_begin (B, K, T) or None.  A score is the
	log-likelihood ratio of the phrase's best alignment on [begin, end] against the greedy path there: 0 at best, not a calibrated probability.
	include/convasr_hip.h (convasr_ctc_keyword_search) has the rule."""
	return ops.ctc_keyword_search(log_probs.float().permute(1, 2, 0), tokens, token_lengths, blank, thresholds, lengths = lengths, min_gap = min_gap, max_hits = max_hits, dense = dense)


def search_bct(log_probs_bct, tokens, token_lengths, blank, thresholds, lengths = None, min_gap: int = 10, max_hits: int = 16, dense: bool = False):
	"""Same for the model's own output layout: logical (B, C, T) whose memory is (B, T, C)."""
	assert ops.is_cl(log_probs_bct)
	return ops.ctc_keyword_search(log_probs_bct, tokens, token_lengths, blank, thresholds, lengths = lengths, min_gap = min_gap, max_hits = max_hits, dense = dense)


STAR_GAP_MODES = ('ends', 'words', 'all')


def star_gaps(targets, ylen, mode, space = None):
	"""Where a star may stand (functional.star_ctc_loss's star_mask): targets (B, S_max), ylen (B,) -> (B, S_max + 1) bool on the targets'
	device, built with elementwise torch ops only (kernel nodes under graph capture).  Gap g lies before label g, gap ylen[b] after the last
	label; entries past ylen[b] are False.  mode: 'ends' -- gaps 0 and ylen (the recording was cut inside speech); 'words' -- the ends and
	the gap before every `space` label (whole words are missing); 'all' -- every gap."""
	if mode not in STAR_GAP_MODES:
		raise ValueError(f'star_gaps: mode {mode!r} is none of {STAR_GAP_MODES}')
	if mode == 'words' and space is None:
		raise ValueError("star_gaps: mode 'words' needs the label of the space")
	if targets.ndim != 2 or ylen.shape != targets.shape[:1]:
		raise ValueError(f'star_gaps: targets (B, S_max) and ylen (B,) expected, got {tuple(targets.shape)}, {tuple(ylen.shape)}')
	S_max = targets.shape[1]
	idx = torch.arange(S_max + 1, device = targets.device).unsqueeze(0)
	n = ylen.to(device = targets.device).unsqueeze(1)
	if mode == 'all':
		return idx <= n
	mask = (idx == 0) | (idx == n)
	if mode == 'words' and S_max > 0:
		label = targets.gather(1, idx.clamp(max = S_max - 1).expand(targets.shape[0], -1))  # label g at gap g (the last column: masked by g < ylen)
		mask = mask | ((label == int(space)) & (idx < n))
	return mask


class StarCTC:
	"""The training option behind JasperNet.ctc_star: every head's CTC loss runs over partial transcripts, with a star allowed in the gaps
	`gaps` names (star_gaps) at the costs `penalty` per frame and `enter` per star used (natural log, <= 0).  The two costs have no
	defaults: the rule is this project's own and nothing has been tuned on speech."""

	def __init__(self, gaps = 'words', *, penalty, enter, space = None):
		if gaps not in STAR_GAP_MODES:
			raise ValueError(f'StarCTC: gaps {gaps!r} is none of {STAR_GAP_MODES}')
		if gaps == 'words' and space is None:
			raise ValueError("StarCTC: gaps = 'words' needs the label of the space")
		for name, v in (('penalty', penalty), ('enter', enter)):
			if not isinstance(v, (int, float)) or isinstance(v, bool) or not v <= 0 or v == float('-inf'):
				raise ValueError(f'StarCTC: {name} must be a finite natural-log cost <= 0, got {v!r}')
		self.gaps, self.penalty, self.enter, self.space = gaps, float(penalty), float(enter), (None if space is None else int(space))

	def mask(self, targets, ylen):
		return star_gaps(targets, ylen, self.gaps, self.space)

	def __repr__(self):
		return f'StarCTC(gaps = {self.gaps!r}, penalty = {self.penalty}, enter = {self.enter}, space = {self.space})'
