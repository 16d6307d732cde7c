"""Forced alignment without a GPU: the numpy restatement of ctc.alignment (tests/_ctc_align_ref.py) against the reference's own outputs
(tests/golden/alignment.npz, alignment_long.npz), against the oracle, and on planted inputs whose path is known; and what
convasr_ctc_alignment_long answers before any launch: its tile queries, its workspace query and its argument envelope.

Every comparison of alignments is exact."""
import ctypes
import os

import numpy as np
import torch

import _ctc_align_ref as R
from oracle import convasr_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
P = ctypes.c_void_p(4096)  # any non-NULL, 16-byte aligned value: never dereferenced


def test_restatement_reproduces_the_reference_golden_alignments():
	g = np.load(os.path.join(GOLDEN, 'alignment.npz'))
	for case in (0, 1, 2):
		k = lambda name: g[f'c{case}/{name}']
		al = R.alignment(k('log_probs'), k('targets'), k('input_lengths'), k('target_lengths'), blank = int(k('blank')))
		assert np.array_equal(al, k('alignment')), case
	g = np.load(os.path.join(GOLDEN, 'alignment_long.npz'))
	al = R.alignment(g['log_probs'], g['targets'], g['input_lengths'], g['target_lengths'], blank = int(g['blank']))
	assert np.array_equal(al, g['alignment']), int((al != g['alignment']).sum())


def test_restatement_equals_the_oracle_on_a_random_ragged_batch():
	gen = torch.Generator().manual_seed(21)
	B, T, S, C = 6, 140, 24, 11
	lp = torch.randn(T, B, C, generator = gen).log_softmax(dim = -1)
	tg = torch.randint(0, C - 1, (B, S), generator = gen)
	il = torch.tensor([T, T - 1, 2 * S + 1, 97, 60, T])
	tl = torch.tensor([S, 1, S, 17, S - 1, 2])
	ref = O.ctc_alignment(lp, tg, il, tl, blank = C - 1)
	al = R.alignment(lp.numpy(), tg.numpy(), il.numpy(), tl.numpy(), blank = C - 1)
	assert np.array_equal(al, ref.numpy())


def test_restatement_returns_the_planted_positions():
	"""1,500 labels over 4,000 frames, boost 6 and boost 12, a padded recording and a full one: 0 labels off."""
	C = 38
	for seed, boost, input_length in ((1, 6.0, None), (2, 12.0, None), (3, 12.0, 3900)):
		lp, tg, pos = R.planted(seed, 4000, 1500, C, C - 1, boost, input_length = input_length)
		assert lp.dtype == np.float32 and np.abs(np.exp(lp.astype(np.float64)).sum(axis = 1) - 1).max() < 1e-5
		assert bool((np.diff(pos) >= 2).all() and (np.diff(pos) <= 3).all()) and not (tg == C - 1).any()
		padded = np.concatenate([tg, np.zeros(7, dtype = np.int64)])
		al = R.alignment_one(lp, padded, input_length or 4000, 1500, blank = C - 1)
		assert np.array_equal(al[:1500], pos), int((al[:1500] != pos).sum())
		assert not al[1500:].any()


def test_alignment_long_tile_and_workspace_queries():
	from convasr_amd import _lib
	lib = _lib.load()
	sb, chunk = lib.convasr_ctc_alignment_long_states_per_block(), lib.convasr_ctc_alignment_long_chunk_frames()
	assert sb >= 128 and sb % 64 == 0 and 16 <= chunk <= 4096
	up = lambda n: (n + 255) // 256 * 256
	for B, T, S in ((1, 1, 1), (3, 1000, 700), (1, 180000, 48000), (2, 1 << 20, 131071)):
		L = 2 * S + 1
		blocks = -(-L // sb)
		want = up(B * T * -(-L // 16) * 4) + up(B * blocks * sb * 4) + up(B * blocks * T * 8)  # back-pointers, carried column, published neighbours
		assert lib.convasr_ctc_alignment_long_workspace_bytes(B, T, S) == want, (B, T, S)
	assert lib.convasr_ctc_alignment_long_workspace_bytes(1, 180000, 48000) < 5 << 30


def test_alignment_long_envelope_is_checked_before_any_launch():
	from convasr_amd import _lib
	lib = _lib.load()
	q = lib.convasr_ctc_alignment_long_workspace_bytes
	for bad, word in (((1, 100, 131072), b'target length'), ((1, (1 << 20) + 1, 10), b'frames'), ((65536, 10, 10), b'batch'), ((0, 10, 10), b'bad arguments'), ((1, 0, 10), b'bad arguments'), ((1, 10, 0), b'bad arguments')):
		assert q(*bad) == -1 and b'ctc_alignment_long' in lib.convasr_last_error() and word in lib.convasr_last_error(), bad
	need = q(2, 100, 40)

	def run(B = 2, T = 100, C = 38, S_max = 40, blank = 37, chunk_frames = 0, ws_bytes = need, lp = P, ws = P):
		return lib.convasr_ctc_alignment_long(lp, P, P, P, P, ws, ws_bytes, B, T, C, S_max, blank, chunk_frames, None)
	for bad, rc in ((dict(S_max = 131072), -3), (dict(T = (1 << 20) + 1), -3), (dict(B = 65536), -3), (dict(chunk_frames = 15), -1), (dict(chunk_frames = 4097), -1), (dict(chunk_frames = -1), -1),
	                (dict(ws_bytes = need - 1), -1), (dict(blank = 38), -1), (dict(C = 1, blank = 0), -1), (dict(lp = None), -1), (dict(ws = ctypes.c_void_p(4100)), -1)):
		assert run(**bad) == rc and b'ctc_alignment_long' in lib.convasr_last_error(), (bad, lib.convasr_last_error())
