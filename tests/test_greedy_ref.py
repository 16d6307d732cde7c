"""The greedy decode's local rule without a GPU: tests/_greedy_ref.py (the restatement the kernel is held against) equals the host loop
GreedyCTCGenerator.generate_host on seeded random paths and on hand-written cases, and convasr_ctc_greedy_segments refuses arguments
outside its envelope before any launch."""
import ctypes
import random

import pytest
import torch

import _greedy_ref as R

P = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced


@pytest.fixture(scope = 'module')
def tok():
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	return CharTokenizerLegacy('ab')


def run_path(rng, T, classes, eps, space):
	"""A path of runs of 1 .. 12 frames; blanks and spaces are as likely as all letters together."""
	path = []
	while len(path) < T:
		c = rng.choice((eps, eps, space, rng.choice(classes), rng.choice(classes)))
		path += [c] * rng.randint(1, 12)
	return path[:T]


def host(tok, paths, lengths, bats, begin, end, ts, **kw):
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	lp = torch.nn.functional.one_hot(torch.tensor(paths), tok.vocab_size).permute(0, 2, 1).float()
	out = GreedyCTCGenerator(bats).generate_host(tok, lp, torch.tensor(begin), torch.tensor(end), output_lengths = lengths, time_stamps = ts, **kw)
	assert all(len(alternatives) == 1 for alternatives in out)
	return [[dict(seg) for seg in alternatives[0]] for alternatives in out]


def restated(tok, paths, lengths, bats, begin, end, ts):
	begin = torch.clamp(torch.tensor(begin), min = 0.0).tolist() if ts is not None else torch.tensor(begin).tolist()
	end = torch.tensor(end).tolist()
	out = []
	for b, path in enumerate(paths):
		tokens, frames, segments = R.greedy_segments(path, lengths[b], tok.eps_id, tok.space_id, bats, split_words = ts is not None)
		out.append(R.segment_dicts(tok, tokens, segments, begin[b], end[b], ts[b].tolist() if ts is not None else None))
	return out


def test_restatement_equals_the_host_loop_on_random_paths(tok):
	rng = random.Random(11)
	classes = (0, 1, 2)
	cases = empty = 0
	for batch in range(60):
		B, T = 40, rng.randint(1, 90)
		bats = (0, 1, 3, 10)[batch % 4]
		paths = [run_path(rng, T, classes, tok.eps_id, tok.space_id) for _ in range(B)]
		paths[0] = [rng.choice((tok.eps_id, tok.space_id)) for _ in range(T)]  # all silence
		lengths = [rng.choice((T, T, rng.randint(0, T))) for _ in range(B)]
		lengths[1] = 0
		begin = [rng.uniform(-1.0, 5.0) for _ in range(B)]
		end = [rng.uniform(5.0, 9.0) for _ in range(B)]
		ts = torch.cumsum(torch.rand(B, T, generator = torch.Generator().manual_seed(batch)), 1) if batch % 2 else None
		want = host(tok, paths, torch.tensor(lengths) if batch % 3 else lengths, bats, begin, end, ts)
		got = restated(tok, paths, lengths, bats, begin, end, ts)
		for b in range(B):
			assert got[b] == want[b], (batch, b, bats, paths[b], lengths[b])
		cases += B
		empty += sum(not w for w in want)
	assert cases >= 2000 and 0 < empty < cases // 2


def S(tok, text):
	return [tok.char2idx[c] for c in text]


HAND = [  # path, n, bats, tokens, frames, segments with split_words, text of every segment
	('||||', 4, 3, '', [], [], []),  # all blank
	('    ', 4, 3, '', [], [], []),  # all space
	('| |a', 3, 3, '', [], [], []),  # only silence before n
	(' |a', 3, 3, 'a', [2], [(0, 2, 2)], ['a']),
	('aa', 2, 3, 'a', [0], [(0, 0, 0)], ['a']),  # a repeat without a blank
	('a|a', 3, 3, 'aa', [0, 2], [(0, 0, 2)], ['aa']),  # ... and with one
	('a||b', 4, 3, 'ab', [0, 3], [(0, 0, 3)], ['ab']),  # bats - 1 blanks
	('a|||b', 5, 3, 'a b', [0, 3, 4], [(0, 0, 4)], ['a b']),  # bats blanks: an inserted space opens no segment
	('a||||b', 6, 3, 'a b', [0, 3, 5], [(0, 0, 5)], ['a b']),  # bats + 1
	('a|b', 3, 0, 'a b', [0, 1, 2], [(0, 0, 2)], ['a b']),  # bats 0 inserts at the first blank, like bats 1
	('a|b', 3, 1, 'a b', [0, 1, 2], [(0, 0, 2)], ['a b']),
	('ab', 2, 0, 'ab', [0, 1], [(0, 0, 1)], ['ab']),
	('a||| b', 6, 3, 'a   b', [0, 3, 4, 4, 5], [(0, 0, 0), (2, 4, 5)], ['a ', '  b']),  # a path space after an inserted one is emitted again
	('a|||', 4, 3, 'a ', [0, 3], [(0, 0, 0)], ['a ']),  # a blank run reaching n
	('a|||b', 4, 3, 'a ', [0, 3], [(0, 0, 0)], ['a ']),  # ... with speech past n
	('a||', 3, 3, 'a', [0], [(0, 0, 0)], ['a']),
	('a  b', 4, 3, 'a  b', [0, 1, 1, 3], [(0, 0, 0), (1, 1, 3)], ['a', '  b']),  # a space from the path stands twice; repeated spaces merge
	('a | b', 5, 3, 'a  b', [0, 1, 1, 4], [(0, 0, 0), (1, 1, 4)], ['a', '  b']),  # a blank after a space is ignored
	('aaa| ', 5, 3, 'a  ', [0, 4, 4], [(0, 0, 0), (1, 4, 4)], ['a', '  ']),  # the end frame is the emitting frame of a repeated class
]


@pytest.mark.parametrize('path, n, bats, tokens, frames, segments, texts', HAND)
def test_hand_written_cases(tok, path, n, bats, tokens, frames, segments, texts):
	got = R.greedy_segments(S(tok, path), n, tok.eps_id, tok.space_id, bats, split_words = True)
	assert got == (S(tok, tokens), frames, segments)
	ts = torch.arange(len(path), dtype = torch.float32).unsqueeze(0) * 0.5
	want = [{'begin': 1.0 + 0.5 * b, 'end': 1.0 + 0.5 * e, 'hyp': text} for (_, b, e), text in zip(segments, texts)]
	assert host(tok, [S(tok, path)], [n], bats, [1.0], [9.0], ts) == [want]
	assert restated(tok, [S(tok, path)], [n], bats, [1.0], [9.0], ts) == [want]
	# without time stamps: one segment, no space doubled
	single = R.greedy_segments(S(tok, path), n, tok.eps_id, tok.space_id, bats, split_words = False)
	assert len(single[2]) == (1 if tokens else 0)
	assert host(tok, [S(tok, path)], [n], bats, [1.0], [9.0], None) == restated(tok, [S(tok, path)], [n], bats, [1.0], [9.0], None)
	if tokens:
		doubled = {first for first, _, _ in segments[1:]}
		assert single[0] == [c for k, c in enumerate(S(tok, tokens)) if k not in doubled]
		assert single[2] == [(0, segments[0][1], segments[-1][2])]


def test_text_key_and_extra_info_pass_through(tok):
	ts = torch.arange(5, dtype = torch.float32).unsqueeze(0)
	out = host(tok, [S(tok, 'a b|a')], [5], 3, [0.0], [1.0], ts, segment_text_key = 'ref', segment_extra_info = [dict(speaker = 2)])
	assert out == [[dict(begin = 0.0, end = 0.0, ref = 'a', speaker = 2), dict(begin = 1.0, end = 4.0, ref = '  ba', speaker = 2)]]


def test_envelope_of_ctc_greedy_segments():
	from convasr_amd import _lib
	lib = _lib.load()
	assert lib.convasr_ctc_greedy_segments_chunk_frames() >= 64
	need = lib.convasr_ctc_greedy_segments_workspace_bytes(2, 10)
	assert need > 0

	def run(B = 2, T = 10, eps = 37, space = 36, bats = 10, split = 1, path = P, lengths = P, tokens = P, frames = P, counts = P, first = P, begin = P, end = P,
	        ws = P, nbytes = need):
		return lib.convasr_ctc_greedy_segments(path, lengths, tokens, frames, counts, first, begin, end, ws, nbytes, B, T, eps, space, bats, split, None)

	for bad in (dict(B = 0), dict(T = 0), dict(B = -1), dict(B = 1 << 16, T = 1 << 15, nbytes = 1 << 40), dict(eps = 5, space = 5), dict(eps = -1), dict(space = -2),
	            dict(bats = -1), dict(path = None), dict(lengths = None), dict(tokens = None), dict(frames = None), dict(counts = None), dict(first = None),
	            dict(begin = None), dict(end = None), dict(ws = None), dict(nbytes = need - 1), dict(nbytes = 0), dict(B = 40)):
		rc = run(**bad)
		assert rc == -1 and b'ctc_greedy_segments' in lib.convasr_last_error(), (bad, rc)
	for bad in ((0, 10), (2, 0), (1 << 16, 1 << 15)):
		assert lib.convasr_ctc_greedy_segments_workspace_bytes(*bad) == -1 and b'ctc_greedy_segments_workspace_bytes' in lib.convasr_last_error(), bad
	assert lib.convasr_ctc_greedy_segments_workspace_bytes(1, (1 << 31) - 1) > 0
