"""Character and word error rates (reference: metrics.py:409-421, cer / wer) with the edit distances on the GPU (convasr_edit_distance).

Two paths:
* strings -- cer / wer / cer_wer: the reference's arithmetic exactly.  CER compares hyp.replace(' ', '').lower() with the same of ref
  (only U+0020 is removed) over Unicode codepoints and divides by len(ref.replace(' ', '')) or 1 of the ref as given (lowercasing can
  change a length: 'İ'.lower() is two codepoints).  WER splits both sides on any whitespace, without lowercasing, maps the words to
  integer ids on the host (the reference's word2char) and divides by len(ref.split()) or 1.  hyp == ref scores 0.  The host prepares
  codepoints / word ids; one launch per metric computes every distance; the ratio is a float64 division of the two integers, as Python's
  int / int is.
* tokens -- token_cer_wer: device tensors of token ids in, device tensors of per-utterance rates out, no host round trip.  It is valid for a
  tokenizer in which every class decodes to one character c with c.lower() == c and only the space class decodes to whitespace
  (CharTokenizerLegacy with the Russian alphabet is one): there it equals the string path applied to tokenizer.decode of the same tokens.
  For any other tokenizer (BPE) decode the tokens and use the string path."""
import numpy as np
import torch

from . import _lib, ops


def _device(device):
	return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def _pack(seqs, device):
	"""Lists of ints -> (N, L) int64 device tensor (zero-padded, L >= 1) and (N,) int64 lengths, one host-to-device copy each."""
	L = max([len(s) for s in seqs] + [1])
	arr = np.zeros((len(seqs), L), dtype = np.int64)
	for i, s in enumerate(seqs):
		arr[i, :len(s)] = s
	lengths = np.array([len(s) for s in seqs], dtype = np.int64)
	return torch.from_numpy(arr).to(device), torch.from_numpy(lengths).to(device)


def char_units(hyps, refs):
	"""The CER inputs of the reference's cer: per pair the codepoints of hyp.replace(' ', '').lower() and of ref.replace(' ', '').lower(), and
	the denominator len(ref.replace(' ', '')) or 1 (before lowercasing)."""
	h = [[ord(c) for c in s.replace(' ', '').lower()] for s in hyps]
	r = [[ord(c) for c in s.replace(' ', '').lower()] for s in refs]
	return h, r, [len(s.replace(' ', '')) or 1 for s in refs]


def word_units(hyps, refs):
	"""The WER inputs of the reference's wer: per pair the word ids of hyp.split() and ref.split() (equal words, equal ids), and the
	denominator len(ref.split()) or 1."""
	ids = {}
	h = [[ids.setdefault(w, len(ids)) for w in s.split()] for s in hyps]
	r = [[ids.setdefault(w, len(ids)) for w in s.split()] for s in refs]
	return h, r, [len(s.split()) or 1 for s in refs]


def _rates(hyp_units, ref_units, denominators, equal, device):
	h, hl = _pack(hyp_units, device)
	r, rl = _pack(ref_units, device)
	dist, _ = ops.edit_distance(h, hl, r, rl, _lib.METRIC_CHARS, -1)
	return [0.0 if same else d / n for d, n, same in zip(dist.cpu().tolist(), denominators, equal)]


def cer_wer(hyps, refs, device = None):
	"""Per-utterance CER and WER of the string pairs (hyps[i], refs[i]), as the reference's metrics.cer / metrics.wer compute them:
	two lists of floats.  Every string's units must number at most 16,383 (ops.edit_distance's envelope)."""
	hyps, refs = list(hyps), list(refs)
	if len(hyps) != len(refs):
		raise ValueError(f'cer_wer: {len(hyps)} hypotheses for {len(refs)} references')
	if not hyps:
		return [], []
	device = _device(device)
	equal = [a == b for a, b in zip(hyps, refs)]
	return _rates(*char_units(hyps, refs), equal, device), _rates(*word_units(hyps, refs), equal, device)


def cer(*, hyp, ref):
	"""metrics.cer (metrics.py:409-411) for one pair, the distance computed on the GPU."""
	return cer_wer([hyp], [ref])[0][0]


def wer(*, hyp, ref):
	"""metrics.wer (metrics.py:414-421) for one pair, the distance computed on the GPU."""
	return cer_wer([hyp], [ref])[1][0]


def token_cer_wer(tokens, lengths, ref, ref_lengths, space):
	"""Per-utterance CER and WER of token hypotheses against token references, on the device.  tokens (B, K, L) int64 with lengths (B, K), or
	(B, L) with (B,); ref (B, Lr) int64 read in place through its row stride (y[:, 0]), ref_lengths (B,) (ylen[:, 0]); space: the space class.
	CER = edit distance over the tokens that are not `space` / (their number in the reference or 1); WER = edit distance over the maximal
	runs of non-space tokens / (their number in the reference or 1).  Returns two float64 device tensors shaped like lengths.  Valid for
	one-character lowercase tokenizers only (see the module docstring)."""
	cd, units = ops.edit_distance(tokens, lengths, ref, ref_lengths, _lib.METRIC_CHARS, int(space))
	wd, words = ops.edit_distance(tokens, lengths, ref, ref_lengths, _lib.METRIC_WORDS, int(space))
	shape = (-1, ) + (1, ) * (cd.ndim - 1)
	return cd.double() / units.clamp(min = 1).double().view(shape), wd.double() / words.clamp(min = 1).double().view(shape)
