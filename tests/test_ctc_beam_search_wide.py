"""The wide CTC beam search without a GPU: the argument envelope of convasr_ctc_beam_search_wide and convasr_ctc_beam_search_lm_wide
(checked before any launch; beam widths up to 8192) and their workspace size, against the formula in include/convasr_hip.h."""
import ctypes

import pytest

P = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced


def _lib():
	from convasr_amd import _lib
	return _lib.load()


def _up(x, a):
	return (x + a - 1) // a * a


def _pow2(x):
	p = 1
	while p < x:
		p <<= 1
	return p


def _wide_bytes(B, T, C, W, N, lm):
	"""The header's formula: the arena (8 bytes per node, rounded up to 256) plus B regions of beam state."""
	NW, MW, TB = (N + 31) // 32, (C + 31) // 32, _pow2(max(2 * W, 64))
	A = _up(68 * W + 4 * W * MW if lm else 52 * W, 16)
	S = _up(2 * A + 24 * W + 4 * W * NW + 4 * TB, 256)
	return _up(8 * B * T * W, 256) + B * S


def test_envelope_of_the_wide_search():
	lib = _lib()
	B, T, C = 2, 10, 38

	def run(W = 8, N = 5, topk = 1, blank = C - 1, cutoff = 1.0, C_ = C, ws = P):
		return lib.convasr_ctc_beam_search_wide(P, P, P, P, P, P, ws, B, T, C_, blank, W, N, cutoff, topk, None)

	for bad in (dict(W = 0), dict(W = 8193), dict(W = 9000, topk = 1), dict(N = 0), dict(N = C + 1), dict(W = 64, N = 129, C_ = 200), dict(C_ = 8193),
	            dict(C_ = 1, blank = 0, N = 1), dict(topk = 9), dict(topk = 0), dict(W = 8192, topk = 8193), dict(blank = C), dict(blank = -1),
	            dict(cutoff = 0.0), dict(cutoff = 1.5), dict(cutoff = float('nan')), dict(ws = None)):
		rc = run(**bad)
		assert rc < 0 and b'ctc_beam_search_wide' in lib.convasr_last_error(), (bad, rc)
	for W in (1, 1025, 5000, 8192):
		assert lib.convasr_ctc_beam_search_wide_workspace_bytes(B, T, C, W, 5, 1) == _wide_bytes(B, T, C, W, 5, False), W
	assert lib.convasr_ctc_beam_search_wide_workspace_bytes(B, T, 8192, 8192, 128, 8192) == _wide_bytes(B, T, 8192, 8192, 128, False)
	for args in ((B, T, C, 0, 5, 1), (B, T, C, 8193, 5, 1), (B, T, C, 8, 129, 1), (B, T, 8193, 8, 5, 1), (B, T, C, 8, 5, 9)):
		assert lib.convasr_ctc_beam_search_wide_workspace_bytes(*args) < 0 and b'ctc_beam_search_wide' in lib.convasr_last_error(), args
	# the arena's index limits: B * T * W < 2^31
	assert lib.convasr_ctc_beam_search_wide_workspace_bytes(64, 4096, C, 8192, 40, 4) < 0
	assert lib.convasr_ctc_beam_search_wide_workspace_bytes(64, 750, C, 5000, 38, 4) == _wide_bytes(64, 750, C, 5000, 38, False)
	# the LDS entry point keeps its envelope
	assert lib.convasr_ctc_beam_search_workspace_bytes(B, T, C, 1025, 5, 1) < 0
	assert lib.convasr_ctc_beam_search_workspace_bytes(B, T, C, 5000, 5, 1) < 0


def test_envelope_of_the_wide_lm_search():
	lib = _lib()
	B, T, C = 2, 10, 38

	def run(W = 8, N = 5, topk = 1, blank = C - 1, cutoff = 1.0, C_ = C, n_nodes = 4, n_ent = 4, n_slots = 8, space = C - 2, order = 3, start = 1,
	        alpha = 0.5, beta = 1.0, ws = P, tab = P):
		return lib.convasr_ctc_beam_search_lm_wide(P, P, P, P, P, P, ws, B, T, C_, blank, W, N, cutoff, topk, tab, P, P, n_nodes, P, P, n_ent, P,
		                                           n_slots, space, order, start, alpha, beta, None)

	for bad in (dict(W = 0), dict(W = 8193), dict(N = 0), dict(N = C + 1), dict(topk = 9), dict(W = 8192, topk = 8193), dict(blank = C),
	            dict(cutoff = 0.0), dict(cutoff = 1.5), dict(C_ = 257, N = 40), dict(C_ = 8193, N = 40), dict(order = 0), dict(order = 7),
	            dict(alpha = float('nan')), dict(beta = float('inf')), dict(space = C - 1), dict(space = C), dict(space = -1), dict(n_nodes = 0),
	            dict(n_ent = 0), dict(n_slots = 6), dict(n_slots = 0), dict(start = -2), dict(start = 4), dict(ws = None), dict(tab = None)):
		rc = run(**bad)
		assert rc < 0 and b'ctc_beam_search_lm_wide' in lib.convasr_last_error(), (bad, rc)
	assert lib.convasr_ctc_beam_search_lm_wide_workspace_bytes(B, T, 257, 8, 5, 1) < 0 and b'256' in lib.convasr_last_error()
	assert lib.convasr_ctc_beam_search_lm_wide_workspace_bytes(B, T, C, 8193, 5, 1) < 0
	# C = 256, N = 128: the LDS form stops at W = 1001, the wide form takes the whole envelope
	assert lib.convasr_ctc_beam_search_lm_workspace_bytes(B, T, 256, 1002, 128, 1) < 0
	for W in (1, 1002, 5000, 8192):
		assert lib.convasr_ctc_beam_search_lm_wide_workspace_bytes(B, T, 256, W, 128, 1) == _wide_bytes(B, T, 256, W, 128, True), W
	assert lib.convasr_ctc_beam_search_lm_wide_workspace_bytes(64, 750, C, 5000, 38, 4) == _wide_bytes(64, 750, C, 5000, 38, True)


@pytest.mark.parametrize('lm', [False, True])
def test_ops_routes_by_the_lds_query(lm):
	"""ops._beam_route: the LDS entry point whenever its query accepts the arguments, the wide one otherwise or when forced."""
	from convasr_amd import _lib as L
	from convasr_amd import ops
	name = 'ctc_beam_search_lm' if lm else 'ctc_beam_search'
	C = 256 if lm else 64
	assert ops._beam_route(name, (2, 10, C, 64, 40, 4), None)[0] == f'convasr_{name}'
	assert ops._beam_route(name, (2, 10, C, 64, 40, 4), True)[0] == f'convasr_{name}_wide'
	assert ops._beam_route(name, (2, 10, C, 5000, 40, 4), None) == (f'convasr_{name}_wide', _wide_bytes(2, 10, C, 5000, 40, lm))
	assert ops._beam_route(name, (2, 10, C, 1024, 40, 4), None) == (f'convasr_{name}', 2 * 10 * 1024 * 8)
	with pytest.raises(L.ConvasrHipError, match = name):
		ops._beam_route(name, (2, 10, C, 5000, 40, 4), False)
	with pytest.raises(L.ConvasrHipError, match = f'{name}_wide'):
		ops._beam_route(name, (2, 10, C, 8193, 40, 4), None)
	if lm:  # the LDS budget at C = 256, N = 128
		assert ops._beam_route(name, (2, 10, 256, 1001, 128, 1), None)[0] == f'convasr_{name}'
		assert ops._beam_route(name, (2, 10, 256, 1002, 128, 1), None)[0] == f'convasr_{name}_wide'
