"""The reference's decoders module (decoders.py:1-55) on the GPU.

* GreedyDecoder: per-frame best class (K = 1: the convasr_argmax kernel), the reference's return form.
* BeamSearchDecoder: CTC prefix beam search (convasr_ctc_beam_search, one workgroup per utterance, the frame loop inside the kernel) in
  place of ctcdecode.CTCBeamDecoder; with lm_path an ARPA n-gram model is fused into the search (convasr_ctc_beam_search_lm, lm.NgramLM)
  as ctcdecode's KenLM scorer is.  A KenLM binary model or any other non-ARPA path raises NotImplementedError.

Scores: ctcdecode documents its beam scores as -log p, so the reference's decoded_scores.topk(topk) would pick the LEAST probable beams of
its output (not verified against an installed ctcdecode).  This module returns the MOST probable beams, best first, and log p itself."""
import math
import os

import torch

from . import hotwords as hot_mod
from . import lm as lm_mod
from . import ops


def _blank_of(labels):
	for name in ('blank_idx', 'eps_id'):  # the reference's Labels / this package's tokenizers
		if getattr(labels, name, None) is not None:
			return int(getattr(labels, name))
	raise ValueError('labels need a blank_idx (reference Labels) or an eps_id (tokenizer) attribute')


def _labels_of(labels):
	"""The label string, one character per class: a str, a tokenizer's idx2char / vocab, a `labels` attribute, or str(labels)."""
	if isinstance(labels, str):
		return labels
	for name in ('idx2char', 'vocab', 'labels'):
		v = getattr(labels, name, None)
		if v is not None and not callable(v):
			if not isinstance(v, str) and not all(isinstance(x, str) and len(x) == 1 for x in v):
				raise ValueError(f'BeamSearchDecoder: the labels {name} are not one character per class: an LM needs character labels')
			return ''.join(v)
	return str(labels)


def _lengths(output_lengths, log_probs):
	return torch.as_tensor(output_lengths if output_lengths is not None else [log_probs.shape[-1]] * len(log_probs)).tolist()


class GreedyDecoder:
	def decode(self, log_probs, output_lengths = None, K = 1):
		"""log_probs (B, C, T).  Returns per utterance the first output_lengths[b] frames' best class (a list of ints), or for K > 1 the
		K best classes per frame (K lists, best first; torch.topk over the class axis, as the reference does).  K = 1 runs the convasr_argmax
		kernel on GPU tensors; a CPU tensor is decoded with torch.argmax on the CPU, as GreedyCTCGenerator and the reference do."""
		if K == 1:
			idx = (ops.argmax(log_probs) if log_probs.is_cuda else log_probs.argmax(dim = 1)).unsqueeze(1)
		else:
			idx = log_probs.topk(K, dim = 1).indices
		return [l[... if K > 1 else 0, :o].tolist() for o, l in zip(_lengths(output_lengths, log_probs), idx)]


class BeamSearchDecoder:
	"""decoders.BeamSearchDecoder.  beam_width <= 8192, cutoff_top_n <= 128 (None or more than C: C), C <= 8192; outside that envelope decode()
	raises.  Widths up to 1024 run the LDS kernel, wider ones (the reference transcribe.py's default --beam-width 5000 among them) the
	wide kernel with the beam state in global memory: the same search, the same results (ops.ctc_beam_search).  num_workers is the reference's CPU thread count and has no
	meaning here.  beam_width is required, as in the reference (it is a keyword here only because lm_path got a default).  The search runs on
	the GPU only: log_probs must be a CUDA tensor.

	lm_path: None (no LM; beam_alpha / beam_beta are ignored), the path of an ARPA text file, or an lm.NgramLM already built for these
	labels (one model for many decoders).  With an LM the labels (a string, or a tokenizer / Labels object whose idx2char, vocab or str()
	gives one character per class, lowercased) need exactly one space, which is not the blank; C <= 256; beam_alpha and beam_beta weigh
	the LM term alpha * ln P(word | context) + beta, and the returned scores are the fused log p (include/convasr_hip.h).  A path that
	cannot be read as ARPA text (a KenLM binary among them) raises NotImplementedError.

	hotwords: None, a list of phrases, or a hotwords.HotWords already built for these labels: the search is biased towards them
	(convasr_ctc_beam_search_hot; ops.ctc_beam_search_hot states the rule).  hotword_weight, in natural-log units per matched label, is
	required whenever hotwords are given: no value has been tuned on speech here, so there is deliberately no default.  The labels need
	exactly one space, which is not the blank; C <= 256; with an LM every word of every phrase must be in its vocabulary; the returned
	scores are then fp64.  Without hotwords nothing changes."""

	def __init__(self, labels, lm_path = None, beam_width = None, beam_alpha = 0, beam_beta = 0, cutoff_top_n = 40, cutoff_prob = 1.0, num_workers = 1, topk = 1,
	             hotwords = None, hotword_weight = None):
		self.lm = self.hot = None
		if lm_path is not None and not isinstance(lm_path, lm_mod.NgramLM):
			arpa = lm_path if isinstance(lm_path, lm_mod.Arpa) else lm_mod.read_arpa(os.fspath(lm_path))  # (NotImplementedError for a non-ARPA path)
			lm_path = lm_mod.NgramLM(arpa, _labels_of(labels))
		if beam_width is None:
			raise TypeError('BeamSearchDecoder: beam_width is required')
		self.blank = _blank_of(labels)
		self.beam_width, self.cutoff_top_n, self.cutoff_prob, self.topk = int(beam_width), cutoff_top_n, float(cutoff_prob), int(topk)
		if lm_path is not None:
			if lm_path.space == self.blank:
				raise ValueError(f'BeamSearchDecoder: the space class {lm_path.space} is the blank')
			self.alpha, self.beta = float(beam_alpha), float(beam_beta)
			if not (math.isfinite(self.alpha) and math.isfinite(self.beta)):
				raise ValueError(f'BeamSearchDecoder: beam_alpha {beam_alpha} and beam_beta {beam_beta} must be finite')
			lm_path.tables(self.blank)  # (the vocabulary's ValueError / NotImplementedError, here rather than at the first decode)
			self.lm = lm_path
		if hotwords is not None:
			if hotword_weight is None:
				raise ValueError('BeamSearchDecoder: hotwords need a hotword_weight (natural-log units per matched label; there is no default)')
			self.hot_weight = float(hotword_weight)
			if not (math.isfinite(self.hot_weight) and self.hot_weight >= 0.0):
				raise ValueError(f'BeamSearchDecoder: hotword_weight {hotword_weight} must be finite and >= 0')
			hot = hotwords if isinstance(hotwords, hot_mod.HotWords) else hot_mod.HotWords(hotwords, _labels_of(labels))
			hot.tables(self.blank)  # (a phrase with the blank's character: ValueError here rather than at the first decode)
			if self.lm is not None:
				hot.check_vocabulary(self.lm, self.blank)
			self.hot = hot
		elif hotword_weight is not None:
			raise ValueError('BeamSearchDecoder: hotword_weight without hotwords')

	def decode_with_scores(self, log_probs, output_lengths = None):
		"""(tokens (B, topk, T) int64, offsets (B, topk, T) int32 frames, lengths (B, topk) int64, log_prob (B, topk)), best first; log_prob is
		fp32 log p without an LM, fp64 fused log p with one, fp64 with hotwords."""
		if self.hot is not None:
			return ops.ctc_beam_search_hot(log_probs, output_lengths, self.blank, self.beam_width, self.hot, self.hot_weight, self.lm, getattr(self, 'alpha', 0.0),
			                               getattr(self, 'beta', 0.0), self.cutoff_top_n, self.cutoff_prob, self.topk)
		if self.lm is not None:
			return ops.ctc_beam_search_lm(log_probs, output_lengths, self.blank, self.beam_width, self.lm, self.alpha, self.beta, self.cutoff_top_n, self.cutoff_prob, self.topk)
		return ops.ctc_beam_search(log_probs, output_lengths, self.blank, self.beam_width, self.cutoff_top_n, self.cutoff_prob, self.topk)

	def decode(self, log_probs, output_lengths = None):
		"""The reference's return form: per utterance the best hypothesis' tokens (topk = 1) or a list of topk token lists, best first."""
		list_or_one = lambda xs: xs if len(xs) > 1 else xs[0]
		tokens, _, lengths, _ = self.decode_with_scores(log_probs, output_lengths)
		tokens, lengths = tokens.cpu(), lengths.cpu().tolist()
		return [list_or_one([d[k, :l[k]].tolist() for k in range(self.topk)]) for d, l in zip(tokens, lengths)]
