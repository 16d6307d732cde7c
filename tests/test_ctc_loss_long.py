"""Host side of convasr_ctc_loss_long (csrc/ctc_long.hip) and of the query that routes ops.ctc_loss: envelopes and argument checks run
before any launch, so none of this needs a GPU."""
import ctypes

from convasr_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3


def test_short_kernel_query_at_its_label_and_frame_limits():
	lib = _lib.load()
	q = lib.convasr_ctc_loss_supported
	assert q(2, 2100, 38, 1023) == 1 and q(2, 2100, 38, 1024) == 0
	assert q(64, 753, 38, 150) == 1 and q(1, 1, 2, 0) == 1
	assert q(2, 2100, 8192, 100) == 1 and q(2, 2100, 8193, 100) == 0
	assert q(0, 753, 38, 150) == 0 and q(2, 0, 38, 150) == 0 and q(2, 753, 1, 150) == 0 and q(2, 753, 38, -1) == 0
	p = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced
	for S in (0, 150, 600, 1023):
		assert q(2, 1, 38, S) == 1
		lo, hi = 1, 1 << 20  # the largest T the short kernel takes: the query is monotone in T
		assert q(2, hi, 38, S) == 0
		while hi - lo > 1:
			mid = (lo + hi) // 2
			lo, hi = (mid, hi) if q(2, mid, 38, S) else (lo, mid)
		assert 11000 < lo < 13100, (S, lo)  # "about 12,000 frames": three hand-over words and a quarter of an offset per frame in 159 KiB of LDS
		assert q(2, lo, 38, S) == 1 and q(2, lo + 1, 38, S) == 0
		# ... and one frame more is what convasr_ctc_loss itself refuses, before any launch
		assert lib.convasr_ctc_loss(p, p, p, p, p, p, p, 2, lo + 1, 38, S, 37, None) < 0 and b'too long' in lib.convasr_last_error()
	assert lib.convasr_ctc_loss(p, p, p, p, p, p, p, 2, 2100, 38, 1024, 37, None) == EUNSUPPORTED and b'1023' in lib.convasr_last_error()


def test_long_workspace_query_at_the_envelope():
	lib = _lib.load()
	w = lib.convasr_ctc_loss_long_workspace_bytes
	SB, CH = lib.convasr_ctc_loss_long_states_per_block(), lib.convasr_ctc_loss_long_chunk_frames()
	assert SB >= 64 and SB % 64 == 0 and 16 <= CH <= 4096
	up = lambda n: (n + 255) // 256 * 256

	def want(B, T, S):
		blocks = (2 * S + 1 + SB - 1) // SB
		return 2 * up(B * T * blocks * SB * 4) + 2 * up(B * blocks * T * 4) + up(8 * B) + up(4 * B)  # two lattices, their per-frame offsets, totals, NaN flags
	for B, T, S in [(2, 2100, 1024), (2, 2100, 1023), (1, 30000, 9000), (3, 120, 1), (1, 1, 0), (5, 2600, 1100)]:
		assert w(B, T, 38, S) == want(B, T, S), (B, T, S)
	assert 4.3e9 < w(1, 30000, 38, 9000) < 4.5e9  # ten minutes: inside the 16 GiB cap
	assert w(1, 1 << 20, 38, 131071) == want(1, 1 << 20, 131071) > (16 << 30)  # the envelope's far corner is a shape, just not one a device holds
	for bad, code, word in [((1, 2100, 38, 131072), EUNSUPPORTED, b'131071'), ((1, (1 << 20) + 1, 38, 100), EUNSUPPORTED, b'frames'), ((1, 2100, 8193, 100), EUNSUPPORTED, b'8192'),
	                        ((65536, 2100, 38, 100), EUNSUPPORTED, b'batch'), ((0, 2100, 38, 100), EINVAL, b'bad arguments'), ((1, 0, 38, 100), EINVAL, b'bad arguments'),
	                        ((1, 2100, 1, 100), EINVAL, b'bad arguments'), ((1, 2100, 38, -1), EINVAL, b'bad arguments')]:
		assert w(*bad) == code and b'ctc_loss_long' in lib.convasr_last_error() and word in lib.convasr_last_error(), (bad, lib.convasr_last_error())
	assert w(1, 1 << 20, 8192, 131071) > 0 and w(65535, 16, 2, 0) > 0 and w(65535, 1 << 20, 38, 131071) == want(65535, 1 << 20, 131071)


def test_long_entry_point_refuses_bad_arguments_before_any_launch():
	lib = _lib.load()
	p = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced
	B, T, C, S = 2, 2100, 38, 1024
	need = lib.convasr_ctc_loss_long_workspace_bytes(B, T, C, S)
	call = lambda **kw: lib.convasr_ctc_loss_long(*[kw.get(k, v) for k, v in dict(lp = p, y = p, olen = p, ylen = p, nll = p, grad = p, ws = p, nbytes = need, B = B, T = T, C = C, S = S, blank = C - 1, chunk = 0, stream = None).items()])
	for kw, word in [(dict(lp = None), b'bad arguments'), (dict(y = None), b'bad arguments'), (dict(olen = None), b'bad arguments'), (dict(ylen = None), b'bad arguments'), (dict(nll = None), b'bad arguments'),
	                 (dict(ws = None), b'bad arguments'), (dict(blank = C), b'bad arguments'), (dict(blank = -1), b'bad arguments'), (dict(B = 0), b'bad arguments'), (dict(C = 1, blank = 0), b'bad arguments'),
	                 (dict(S = 131072), b'131071'), (dict(T = (1 << 20) + 1), b'frames'), (dict(C = 8193), b'8192'), (dict(B = 65536), b'batch'),
	                 (dict(chunk = 15), b'chunk_frames'), (dict(chunk = 4097), b'chunk_frames'), (dict(chunk = -1), b'chunk_frames'),
	                 (dict(nbytes = need - 1), str(need).encode()), (dict(ws = ctypes.c_void_p(4100)), b'aligned')]:
		assert call(**kw) < 0, kw
		assert b'ctc_loss_long' in lib.convasr_last_error() and word in lib.convasr_last_error(), (kw, lib.convasr_last_error())


def test_ops_route_and_tiles_are_exported():
	from convasr_amd import ops
	assert ops.CTC_LONG_WORKSPACE_CAP == 16 << 30
	lib = _lib.load()
	assert ops.ctc_loss_long_tiles() == (lib.convasr_ctc_loss_long_states_per_block(), lib.convasr_ctc_loss_long_chunk_frames())
	assert lib.convasr_abi_version() == 11
