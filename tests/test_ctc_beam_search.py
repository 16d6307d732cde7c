"""CTC prefix beam search without a GPU: the float64 restatement (tests/_ctc_beam_ref.py) against brute force, the argument envelope of
convasr_ctc_beam_search (checked before any launch), and the decoder's refusal of a language model."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctc_beam_ref as R  # noqa: E402


def _log_softmax(x):
	return x - np.logaddexp.reduce(x, axis = -1, keepdims = True)


def _labellings(L, C, blank):
	out = set()
	for path in itertools.product(range(C), repeat = L):
		lab, prev = [], None
		for c in path:
			if c != blank and c != prev:
				lab.append(c)
			prev = c
		out.add(tuple(lab))
	return out


def test_restatement_against_brute_force():
	"""W above the number of reachable prefixes and N = C: nothing is pruned, so every returned labelling's log-probability is the
	exhaustive sum over its CTC paths, every reachable labelling is returned, and the top one is the most probable."""
	rng = np.random.default_rng(1234)
	for _ in range(40):
		L, C = int(rng.integers(1, 7)), int(rng.integers(2, 5))
		if C ** L > 5000:
			L = 4
		lp = _log_softmax(rng.normal(size = (L, C)) * 2.0)
		blank = int(rng.integers(0, C))
		labs = _labellings(L, C, blank)
		W = len(labs) + 3
		hyps, _ = R.decode_one(lp, blank, W, C, 1.0, W)
		assert len(hyps) == len(labs)
		exact = {lab: R.labelling_log_prob(lp, lab, blank) for lab in labs}
		for toks, offs, s in hyps:
			assert abs(exact[tuple(toks)] - s) <= 1e-12, (toks, exact[tuple(toks)], s)
			assert offs == sorted(offs) and all(0 <= o < L for o in offs)
		assert tuple(hyps[0][0]) == max(labs, key = exact.get)
		assert [h[2] for h in hyps] == sorted((h[2] for h in hyps), reverse = True)


def test_restatement_empty_and_pruned():
	"""L = 0 gives one empty hypothesis of log-probability 0; W = 1, N = 1 is the greedy path collapsed."""
	hyps, _ = R.decode_one(np.zeros((0, 5)), 4, 8, 5, 1.0, 3)
	assert hyps == [([], [], 0.0)]
	rng = np.random.default_rng(7)
	lp = _log_softmax(rng.normal(size = (30, 6)) * 3.0)
	best = lp.argmax(-1)
	want, prev = [], None
	for c in best:
		if c != 5 and c != prev:
			want.append(int(c))
		prev = c
	hyps, _ = R.decode_one(lp, 5, 1, 1, 1.0, 1)
	assert hyps[0][0] == want and abs(hyps[0][2] - lp[np.arange(30), best].sum()) < 1e-12


def test_argument_envelope_of_ctc_beam_search_is_checked_before_any_launch():
	from convasr_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced
	B, T, C = 2, 10, 38

	def run(W = 8, N = 5, topk = 1, blank = C - 1, cutoff = 1.0, C_ = C):
		return lib.convasr_ctc_beam_search(p, p, p, p, p, p, p, B, T, C_, blank, W, N, cutoff, topk, None)

	for bad in (dict(W = 0), dict(W = 1025), dict(W = 5000), dict(N = C + 1), dict(N = 0), dict(topk = 9), dict(topk = 0), dict(blank = C), dict(blank = -1),
	            dict(cutoff = 0.0), dict(cutoff = 1.5), dict(cutoff = float('nan')), dict(C_ = 1, blank = 0, N = 1), dict(C_ = 8193, N = 5), dict(W = 64, N = 129, C_ = 200)):
		rc = run(**bad)
		assert rc < 0 and b'ctc_beam_search' in lib.convasr_last_error(), (bad, rc)
	assert lib.convasr_ctc_beam_search_workspace_bytes(B, T, C, 1025, 5, 1) < 0 and b'ctc_beam_search' in lib.convasr_last_error()
	assert lib.convasr_ctc_beam_search_workspace_bytes(64, 750, C, 1024, 38, 4) == 64 * 750 * 1024 * 8
	assert lib.convasr_ctc_beam_search(p, p, p, p, p, p, None, B, T, C, C - 1, 8, 5, 1.0, 1, None) < 0  # NULL workspace


def test_beam_search_decoder_refuses_a_language_model():
	import types
	from convasr_amd import decoders, transcript_generators
	with pytest.raises(NotImplementedError, match = 'language-model'):
		decoders.BeamSearchDecoder(types.SimpleNamespace(blank_idx = 0), lm_path = 'x.arpa', beam_width = 8)
	with pytest.raises(NotImplementedError):
		transcript_generators.BeamCTCGenerator(beam_width = 8, lm_path = 'x.arpa')
	assert decoders.BeamSearchDecoder(types.SimpleNamespace(eps_id = 37), beam_width = 8, beam_alpha = 0.4, beam_beta = 2.6).blank == 37


def test_decoders_without_a_gpu():
	"""GreedyDecoder decodes CPU tensors (K = 1: torch.argmax, as the reference); BeamSearchDecoder needs a beam width, as the reference does."""
	import types
	import torch
	from convasr_amd import decoders
	rng = np.random.default_rng(3)
	lp = torch.from_numpy(_log_softmax(rng.normal(size = (3, 20, 6))).astype(np.float32)).permute(0, 2, 1)
	olen = [20, 7, 0]
	for K in (1, 2):
		want = [l[... if K > 1 else 0, :o].tolist() for o, l in zip(olen, lp.topk(K, dim = 1).indices)]
		assert decoders.GreedyDecoder().decode(lp, olen, K = K) == want
	with pytest.raises(TypeError, match = 'beam_width'):
		decoders.BeamSearchDecoder(types.SimpleNamespace(blank_idx = 5))
