"""Host side of convasr_nw_align_long / convasr_edit_distance_long (csrc/nw_long.hip) and of the routing above them in metrics.py:
envelopes and argument checks run before any launch, and the routing is plain Python, so none of this needs a GPU."""
import ctypes
import os
import re

import pytest

from convasr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
NEW = ['convasr_nw_align_long_tile', 'convasr_nw_align_long_workspace_bytes', 'convasr_nw_align_long', 'convasr_nw_align_long_parts',
       'convasr_edit_distance_long_workspace_bytes', 'convasr_edit_distance_long']


def test_entries_are_declared_and_the_abi_is_11():
	header = open(os.path.join(ROOT, 'include', 'convasr_hip.h')).read()
	lib = _lib.load()
	for name in NEW:
		assert re.search(r'\b' + name + r'\s*\(', header), name
		assert name in _lib._SIGNATURES and hasattr(lib, name), name
	assert 'CONVASR_ABI_VERSION 11' in header and lib.convasr_abi_version() == 11
	integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
	for name in NEW:
		assert name in integration, name


def test_tile_is_a_multiple_of_64():
	from convasr_amd import ops
	T = _lib.load().convasr_nw_align_long_tile()
	assert T >= 64 and T % 64 == 0 and ops.nw_align_long_tile() == T
	assert ops.NW_LONG_WORKSPACE_CAP == 16 << 30 and ops.NW_LONG_MAX_LEN == 131071


def test_workspace_queries_equal_the_formula_of_the_header():
	lib = _lib.load()
	T = lib.convasr_nw_align_long_tile()
	up = lambda n: (n + 255) // 256 * 256
	tiles = lambda L: (L + T - 1) // T
	bounds = lambda N, La, Lb: up(N * tiles(La) * (Lb + 1) * 4) + up(N * tiles(Lb) * (La + 1) * 4)
	align = lambda N, La, Lb: up(N * tiles(La) * tiles(Lb) * T * T // 4) + bounds(N, La, Lb) + up(N * max(tiles(La), tiles(Lb), 1) * 8) + up(N * (La + Lb) * 8)
	for shape in [(1, 0, 0), (1, 1, 1), (3, T, T + 1), (1, 131071, 131071), ((1 << 20) - 1, 1, 1), (2, 0, 700), (5, 3 * T - 1, 2 * T)]:
		assert lib.convasr_nw_align_long_workspace_bytes(*shape) == align(*shape), shape
		assert lib.convasr_edit_distance_long_workspace_bytes(*shape) == bounds(*shape), shape
	assert lib.convasr_nw_align_long_workspace_bytes(1, 0, 0) == 256  # (the end-cell key of the one pair, rounded up)
	assert 4 << 30 <= lib.convasr_nw_align_long_workspace_bytes(1, 131071, 131071) < 5 << 30
	assert 2 * 268e6 < lib.convasr_edit_distance_long_workspace_bytes(1, 131071, 131071) < 2 * 269e6
	for bad in [(0, 5, 5), (1 << 20, 5, 5), (1, -1, 5), (1, 5, -1), (1, 131072, 5), (1, 5, 131072)]:
		for query, word in ((lib.convasr_nw_align_long_workspace_bytes, b'nw_align_long'), (lib.convasr_edit_distance_long_workspace_bytes, b'edit_distance_long')):
			assert query(*bad) == -1 and word in lib.convasr_last_error(), bad


def test_entry_points_refuse_bad_arguments_before_any_launch():
	lib = _lib.load()
	p = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced
	N, La, Lb = 2, 700, 300
	need = lib.convasr_nw_align_long_workspace_bytes(N, La, Lb)
	names = ['a', 'al', 'b', 'bl', 'ai', 'bi', 'n', 'score', 'ws']
	base = dict({k: p for k in names}, nbytes = need, N = N, La = La, Lb = Lb, match = 5, sub = -3, dele = -4, ins = -3, stream = None)
	call = lambda **kw: lib.convasr_nw_align_long(*[kw.get(k, v) for k, v in base.items()])
	cases = [(dict({k: None}), EINVAL, b'NULL') for k in names]
	cases += [(dict({k: v}), EINVAL, b'2048') for k in ('match', 'sub', 'dele', 'ins') for v in (2049, -2049)]
	cases += [(dict(nbytes = need - 1), EINVAL, str(need).encode()), (dict(ws = ctypes.c_void_p(4100)), EINVAL, b'aligned'), (dict(N = 0), EINVAL, b'pairs'),
	          (dict(N = 1 << 20), EINVAL, b'pairs'), (dict(La = -1), EINVAL, b'>= 0'), (dict(La = 131072), EUNSUPPORTED, b'131071'), (dict(Lb = 131072), EUNSUPPORTED, b'131071')]
	for kw, code, word in cases:
		assert call(**kw) == code, kw
		assert b'nw_align_long' in lib.convasr_last_error() and word in lib.convasr_last_error(), (kw, lib.convasr_last_error())
	parts = lambda v: lib.convasr_nw_align_long_parts(*list(base.values())[:-1], v, None)
	assert parts(0) == EINVAL and parts(4) == EINVAL and b'parts' in lib.convasr_last_error()

	need = lib.convasr_edit_distance_long_workspace_bytes(N, La, Lb)
	names = ['a', 'al', 'b', 'bl', 'dist', 'ws']
	base = dict({k: p for k in names}, nbytes = need, N = N, La = La, Lb = Lb, stream = None)
	call = lambda **kw: lib.convasr_edit_distance_long(*[kw.get(k, v) for k, v in base.items()])
	cases = [(dict({k: None}), EINVAL, b'NULL') for k in names]
	cases += [(dict(nbytes = need - 1), EINVAL, str(need).encode()), (dict(ws = ctypes.c_void_p(4100)), EINVAL, b'aligned'), (dict(N = 0), EINVAL, b'pairs'),
	          (dict(Lb = -1), EINVAL, b'>= 0'), (dict(La = 131072), EUNSUPPORTED, b'131071')]
	for kw, code, word in cases:
		assert call(**kw) == code, kw
		assert b'edit_distance_long' in lib.convasr_last_error() and word in lib.convasr_last_error(), (kw, lib.convasr_last_error())


def test_routing_split_by_envelope_and_by_request():
	from convasr_amd import metrics
	la, lb = [0, 16383, 16384, 5, 16383, 131071], [7, 16383, 5, 16384, 1, 2]
	assert metrics.split_route(la, lb) == ([0, 1, 4], [2, 3, 5])
	assert metrics.split_route(la, lb, 'short') == (list(range(6)), [])
	assert metrics.split_route(la, lb, 'long') == ([], list(range(6)))
	with pytest.raises(ValueError):
		metrics.split_route(la, lb, 'tiled')


def test_routes_reach_their_launchers_with_their_own_pairs():
	import torch
	from convasr_amd import metrics
	seqs_a = [[1] * 3, [2] * 16384, [3] * 10, [4] * 2]
	seqs_b = [[1] * 4, [2] * 5, [3] * 16383, [4] * 16385]
	calls = []

	def short_fn(h, hl, r, rl, mode, space):
		calls.append(('short', hl.tolist(), rl.tolist(), h.dtype, mode, space))
		return (hl + 100 * rl).to(torch.int32), None

	def long_fn(h, hl, r, rl):
		calls.append(('long', hl.tolist(), rl.tolist(), h.dtype))
		return (hl + 100 * rl).to(torch.int32)
	got = metrics._distances(seqs_a, seqs_b, 'cpu', None, short_fn, long_fn)
	assert got == [len(a) + 100 * len(b) for a, b in zip(seqs_a, seqs_b)]
	assert calls == [('short', [3, 10], [4, 16383], torch.int64, _lib.METRIC_CHARS, -1), ('long', [16384, 2], [5, 16385], torch.int32)]
	calls.clear()
	metrics._distances(seqs_a[:1], seqs_b[:1], 'cpu', None, short_fn, long_fn)
	assert [c[0] for c in calls] == ['short']  # a batch inside the old envelope makes the one call it always made

	def fake_align(tag):
		def fn(a, al, b, bl, scores):
			calls.append((tag, al.tolist(), bl.tolist(), tuple(a.shape), tuple(b.shape), scores))
			N, W = a.shape[0], a.shape[1] + b.shape[1]
			idx = torch.arange(W, dtype = torch.int32).repeat(N, 1)
			return idx, idx + 1000, (al + bl).to(torch.int32), torch.zeros(N, dtype = torch.int32)
		return fn
	calls.clear()
	got = metrics.gpu_aligner(seqs_a, seqs_b, (5, -3, -4, -3), 'cpu', None, fake_align('short'), fake_align('long'))
	assert calls == [('short', [3, 10], [4, 16383], (2, 10), (2, 16383), (5, -3, -4, -3)), ('long', [16384, 2], [5, 16385], (2, 16384), (2, 16385), (5, -3, -4, -3))]
	for (ai, bi), a, b in zip(got, seqs_a, seqs_b):
		assert ai == list(range(len(a) + len(b))) and bi == [k + 1000 for k in ai]
	calls.clear()
	metrics.gpu_aligner(seqs_a, seqs_b, (1, 0, 0, 0), 'cpu', 'long', fake_align('short'), fake_align('long'))
	assert [c[0] for c in calls] == ['long'] and calls[0][1] == [3, 16384, 10, 2]


def test_grouping_under_a_cap():
	from convasr_amd import ops
	lib = _lib.load()
	need = lib.convasr_nw_align_long_workspace_bytes
	la, lb = [300, 10, 5000, 4000, 20, 4900, 0], [200, 10, 5100, 100, 4000, 5000, 0]
	whole = need(len(la), max(la), max(lb))
	big = need(1, 5000, 5100)
	assert ops._cap_groups(la, lb, need, whole) == [(sorted(range(len(la)), key = lambda p: -need(1, la[p], lb[p])), 5000, 5100)]  # under the cap: one group
	groups = ops._cap_groups(la, lb, need, big)
	assert groups[0] == ([2], 5000, 5100) and len(groups) >= 2  # the largest pair first, alone: a second one of its size would not fit
	assert sorted(p for members, _, _ in groups for p in members) == list(range(len(la)))
	for members, ga, gb in groups:
		assert ga == max(la[p] for p in members) and gb == max(lb[p] for p in members) and need(len(members), ga, gb) <= big
	# the fewest groups of this greedy order: a group closes only when the next pair does not fit into it
	order = [p for members, _, _ in groups for p in members]
	assert order == sorted(range(len(la)), key = lambda p: -need(1, la[p], lb[p]))
	for (members, ga, gb), (nxt, na, nb) in zip(groups, groups[1:]):
		assert need(len(members) + 1, max(ga, la[nxt[0]]), max(gb, lb[nxt[0]])) > big
	assert ops._cap_groups(la, lb, need, big - 1)[0] == ([2], 5000, 5100)  # one pair over the cap still comes back, first: the caller raises


def test_nw_align_splits_by_the_library_query_as_it_did_by_its_formula():
	"""ops.nw_align sizes the groups of a batch over its cap with convasr_nw_align_workspace_bytes; it used to size them with the formula
	the header states for that query, written out in Python.  The two are the same function, so the split -- groups and launches -- of
	the batch tests/test_align_gpu.py::test_split_over_the_workspace_cap runs is the same."""
	import random
	from convasr_amd import ops
	formula = lambda n, la, lb: n * (la * ((lb + 63) // 64) * 16 + (la + lb) * 4)
	for shape in [(1, 0, 0), (1, 700, 650), (150, 199, 199), (7, 64, 65), (1, 16383, 16383)]:
		assert _lib.load().convasr_nw_align_workspace_bytes(*shape) == ops.nw_align_workspace_bytes(*shape) == formula(*shape), shape
	rng = random.Random(10)
	seq = lambda n: [rng.randrange(3) for _ in range(n)]
	pairs = [(seq(rng.randrange(0, 200)), seq(rng.randrange(0, 200))) for _ in range(150)] + [(seq(700), seq(650))]
	rng.shuffle(pairs)
	la, lb = [len(a) for a, b in pairs], [len(b) for a, b in pairs]
	cap = 400_000
	groups = ops._cap_groups(la, lb, ops.nw_align_workspace_bytes, cap)
	assert groups == ops._cap_groups(la, lb, formula, cap)
	assert 2 <= len(groups) < 20 and groups[0][1:] == (700, 650) and all(formula(len(members), ga, gb) <= cap for members, ga, gb in groups)
