"""Host mirror of the reference's ctc.py: forced alignment on the GPU; and this package's own keyword search (`search`)."""
import types

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

	def align(self, log_probs_bct, targets, input_lengths, target_lengths, blank, chunk_frames: int = 0):
		"""star_alignment_bct with this object's gaps and costs: where every label of a partial transcript lies in the recording, and which
		frames the star of every gap absorbed."""
		targets = targets.to(log_probs_bct.device)
		return star_alignment_bct(log_probs_bct, targets, input_lengths, target_lengths, blank, self.mask(targets, target_lengths.to(targets.device)), self.penalty, self.enter, chunk_frames = chunk_frames)

	def __repr__(self):
		return f'StarCTC(gaps = {self.gaps!r}, penalty = {self.penalty}, enter = {self.enter}, space = {self.space})'


def star_alignment(log_probs, targets, input_lengths, target_lengths, blank, star_mask, penalty, enter, chunk_frames: int = 0):
	"""Align a PARTIAL transcript to a whole recording (this package's own; the rule is unpinned against any outside aligner and the costs
	are untuned): the best path through star_ctc_loss's lattice -- a star, "any stretch of frames, or nothing", in every gap star_mask
	allows (star_gaps) at `penalty` per frame and `enter` per star used.  log_probs (T, B, C) as `alignment` takes them.  Returns
	ops.star_ctc_alignment's namespace: alignment (B, S_max) like `alignment`, star_begin / star_frames (B, S_max + 1) -- the frames gap g's
	star absorbed: audio the transcript does not cover --, score (B,).  Up to 131,071 labels over 2^20 frames.  True max-plus Viterbi, not
	`alignment`'s log-sum-exp recursion: with an all-false mask the two agree wherever the best path is unambiguous.  A star absorbs audio,
	not text: words in the transcript that were never spoken are not handled.  include/convasr_hip.h (convasr_star_alignment) has the rule."""
	return ops.star_ctc_alignment(log_probs.float().permute(1, 0, 2).contiguous(), targets, input_lengths, target_lengths, blank, star_mask, penalty, enter, chunk_frames = chunk_frames)


def star_alignment_bct(log_probs_bct, targets, input_lengths, target_lengths, blank, star_mask, penalty, enter, chunk_frames: int = 0):
	"""Same for the model's own output layout: logical (B, C, T) whose memory is (B, T, C)."""
	assert ops.is_cl(log_probs_bct)
	return ops.star_ctc_alignment(log_probs_bct.permute(0, 2, 1).float().contiguous(), targets, input_lengths, target_lengths, blank, star_mask, penalty, enter, chunk_frames = chunk_frames)


def star_pieces(result, targets, target_lengths, min_star_frames):
	"""What a cutter would write from a star alignment (host code over the small outputs).  result: star_alignment's namespace (its
	input_lengths are read too); targets (B, S_max), target_lengths (B,).  Per utterance a namespace of
	  stars: the used stars of at least min_star_frames frames, as (gap, begin_frame, end_frame), end inclusive;
	  pieces: the stretches of the transcript between them, as (first_label, label_count, begin_frame, end_frame): a piece begins on the
	    first frame after the star before it (the first piece: frame 0) and ends on the last frame before the star after it (the last piece:
	    frame Tb - 1 = input_lengths[b] - 1).  A stretch without labels is no piece.
	An utterance without a path (score -inf) has neither."""
	begin, frames, score = (t.detach().cpu().tolist() for t in (result.star_begin, result.star_frames, result.score))
	ylen = [int(n) for n in target_lengths.tolist()]
	olen = [int(n) for n in result.input_lengths.tolist()]
	out = []
	for b, S in enumerate(ylen):
		stars, pieces = [], []
		if score[b] != float('-inf'):
			stars = [(g, begin[b][g], begin[b][g] + frames[b][g] - 1) for g in range(S + 1) if frames[b][g] >= max(1, int(min_star_frames))]
			first, at = 0, 0
			for g, lo, hi in stars + [(S, None, None)]:
				if g > first:
					last = lo - 1 if lo is not None else olen[b] - 1
					pieces.append((first, g - first, at, last))
				if hi is not None:
					first, at = g, hi + 1
		out.append(types.SimpleNamespace(stars = stars, pieces = pieces))
	return out


MWER_UNITS = ('words', 'chars')


class MWER:
	"""The training option behind JasperNet.ctc_mwer: in train() mode head `head` also gets the N-best minimum-word-error-rate term
	(functional.mwer_loss; include/convasr_hip.h: convasr_mwer_loss has the rule) and the step's loss becomes ctc_weight * the plain loss +
	weight * mwer_loss.  The N-best list is decoded from the detached log-probs of the same step (ops.ctc_beam_search at beam_width, topk =
	n_best) and every hypothesis is scored against the reference by ops.edit_distance in `unit`s ('words' needs the label of the space).
	include_reference: where no hypothesis equals the reference, the last slot becomes the reference with risk 0.  weight and ctc_weight
	have no defaults: the rule is this project's own, nothing has been tuned on speech, and no effect on word error rate is shown."""

	def __init__(self, n_best, beam_width, weight, ctc_weight, unit = 'words', space = None, scale = 1.0, include_reference = False, head = 0):
		n_best, beam_width = int(n_best), int(beam_width)
		max_hyps = ops.mwer_tiles()[3]
		if not 2 <= n_best <= max_hyps:
			raise ValueError(f'MWER: n_best {n_best} is outside [2, {max_hyps}] (one hypothesis has no gradient)')
		if beam_width < n_best:
			raise ValueError(f'MWER: beam_width {beam_width} is below n_best {n_best}')
		if unit not in MWER_UNITS:
			raise ValueError(f'MWER: unit {unit!r} is none of {MWER_UNITS}')
		if unit == 'words' and space is None:
			raise ValueError("MWER: unit = 'words' needs the label of the space")
		for name, v in (('weight', weight), ('ctc_weight', ctc_weight)):
			if not isinstance(v, (int, float)) or isinstance(v, bool) or not 0 <= v < float('inf'):
				raise ValueError(f'MWER: {name} must be a finite number >= 0, got {v!r}')
		if not isinstance(scale, (int, float)) or isinstance(scale, bool) or not 0 < scale < float('inf'):
			raise ValueError(f'MWER: scale must be a finite number > 0, got {scale!r}')
		self.n_best, self.beam_width, self.weight, self.ctc_weight = n_best, beam_width, float(weight), float(ctc_weight)
		self.unit, self.space, self.scale = unit, (None if space is None else int(space)), float(scale)
		self.include_reference, self.head = bool(include_reference), int(head)
		self.skipped = None  # of the last hypotheses() call: how many utterances had a hypothesis past the kernel's envelope (0-d int64 on the device)

	def hypotheses(self, log_probs, olen, y, ylen, blank = None):
		"""log_probs (B, C, T) of one head, olen (B,), references y (B, Lr) with ylen (B,) -> (hyps (B, n_best, L) int64, hyp_lengths (B,
		n_best) int64 with -1 for an absent hypothesis, risk (B, n_best) fp32), on the device.  A slot the search could not fill is absent;
		an utterance with a hypothesis of more than convasr_mwer_max_labels() labels has all of them absent and is counted in self.skipped.
		blank: the last class by default, as in the model."""
		max_labels = ops.mwer_tiles()[2]
		with torch.no_grad():
			lp = log_probs.detach()
			blank = lp.shape[1] - 1 if blank is None else int(blank)
			tokens, _, lengths, score = ops.ctc_beam_search(lp, olen, blank, self.beam_width, topk = self.n_best)
			L = max(int(lengths.max()), 1)
			hyps = tokens[:, :, :L]
			lengths = torch.where(score == float('-inf'), torch.full_like(lengths, -1), lengths)
			y, ylen = y.to(device = lp.device, dtype = torch.int64), ylen.to(device = lp.device, dtype = torch.int64)
			if self.unit == 'words':
				distance, _ = ops.edit_distance(hyps, lengths.clamp(min = 0), y, ylen, ops._lib.METRIC_WORDS, self.space)
			else:
				distance, _ = ops.edit_distance(hyps, lengths.clamp(min = 0), y, ylen, ops._lib.METRIC_CHARS)
			risk = distance.to(torch.float32)
			if self.include_reference:
				Lr = y.shape[1]
				if Lr > L:
					hyps = torch.nn.functional.pad(hyps, (0, Lr - L))
				ref = torch.nn.functional.pad(y, (0, hyps.shape[2] - Lr))
				idx = torch.arange(hyps.shape[2], device = lp.device)
				same = (lengths == ylen.unsqueeze(1)) & ((hyps == ref.unsqueeze(1)) | (idx >= ylen.view(-1, 1, 1))).all(dim = 2)
				put = ~same.any(dim = 1)  # (B,): the reference is not in the list
				hyps = hyps.clone()
				hyps[:, -1] = torch.where(put.unsqueeze(1), ref, hyps[:, -1])
				lengths = lengths.clone()
				lengths[:, -1] = torch.where(put, ylen, lengths[:, -1])
				risk[:, -1] = torch.where(put, torch.zeros_like(risk[:, -1]), risk[:, -1])
			long = (lengths > max_labels).any(dim = 1)
			self.skipped = long.sum()
			lengths = torch.where(long.unsqueeze(1), torch.full_like(lengths, -1), lengths)
			hyps = hyps[:, :, :max_labels].contiguous()
		return hyps, lengths, risk

	def __repr__(self):
		return (f'MWER(n_best = {self.n_best}, beam_width = {self.beam_width}, weight = {self.weight}, ctc_weight = {self.ctc_weight}, unit = {self.unit!r}, space = {self.space}, '
		        f'scale = {self.scale}, include_reference = {self.include_reference}, head = {self.head})')
