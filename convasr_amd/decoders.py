"""The reference's decoders module (decoders.py:1-55) on the GPU.

* GreedyDecoder: per-frame best class (K = 1: the convasr_argmax kernel), the reference's return form.
* BeamSearchDecoder: CTC prefix beam search without a language model (convasr_ctc_beam_search, one workgroup per utterance, the frame
  loop inside the kernel) in place of ctcdecode.CTCBeamDecoder.  No LM scorer exists here: lm_path must be None.

Scores: ctcdecode documents its beam scores as -log p, so the reference's decoded_scores.topk(topk) would pick the LEAST probable beams of
its output (not verified against an installed ctcdecode).  This module returns the MOST probable beams, best first, and log p itself."""
import torch

from . import ops


def _blank_of(labels):
	for name in ('blank_idx', 'eps_id'):  # the reference's Labels / this package's tokenizers
		if getattr(labels, name, None) is not None:
			return int(getattr(labels, name))
	raise ValueError('labels need a blank_idx (reference Labels) or an eps_id (tokenizer) attribute')


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
	"""decoders.BeamSearchDecoder without a language model.  beam_width <= 1024, cutoff_top_n <= 128 (None or more than C: C), C <= 8192; outside
	that envelope decode() raises (the reference transcribe.py's default --beam-width 5000 among them).  beam_alpha / beam_beta weigh the
	LM and are ignored; num_workers is the reference's CPU thread count and has no meaning here.  beam_width is required, as in the reference
	(it is a keyword here only because lm_path got a default).  The search runs on the GPU only: log_probs must be a CUDA tensor."""

	def __init__(self, labels, lm_path = None, beam_width = None, beam_alpha = 0, beam_beta = 0, cutoff_top_n = 40, cutoff_prob = 1.0, num_workers = 1, topk = 1):
		if lm_path is not None:
			raise NotImplementedError(f'BeamSearchDecoder: lm_path = {lm_path!r}, but there is no language-model scorer in convasr_amd (LM-free beam search only)')
		if beam_width is None:
			raise TypeError('BeamSearchDecoder: beam_width is required')
		self.blank = _blank_of(labels)
		self.beam_width, self.cutoff_top_n, self.cutoff_prob, self.topk = int(beam_width), cutoff_top_n, float(cutoff_prob), int(topk)

	def decode_with_scores(self, log_probs, output_lengths = None):
		"""(tokens (B, topk, T) int64, offsets (B, topk, T) int32 frames, lengths (B, topk) int64, log_prob (B, topk) fp32), best first."""
		return ops.ctc_beam_search(log_probs, output_lengths, self.blank, self.beam_width, self.cutoff_top_n, self.cutoff_prob, self.topk)

	def decode(self, log_probs, output_lengths = None):
		"""The reference's return form: per utterance the best hypothesis' tokens (topk = 1) or a list of topk token lists, best first."""
		list_or_one = lambda xs: xs if len(xs) > 1 else xs[0]
		tokens, _, lengths, _ = self.decode_with_scores(log_probs, output_lengths)
		tokens, lengths = tokens.cpu(), lengths.cpu().tolist()
		return [list_or_one([d[k, :l[k]].tolist() for k in range(self.topk)]) for d, l in zip(tokens, lengths)]
