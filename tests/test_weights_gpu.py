"""convasr_amd.weights on the MI355X: every kind of derived parameter copy goes through one registry and one staleness rule -- made on first
use, refreshed in place when (and only when) the parameter's version moved, re-made after force_repack(), dropped together with the
reference to its parameter by invalidate_pack_cache() -- and the arena's 16-bit mirror serves as the packed forward copy once it is
vouched for.  Shapes: the smallest at which each kind exists."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _padded_head(w):
	from convasr_amd import weights as W
	wp = torch.zeros(W.HEAD_PAD, w.shape[1], 1, device = w.device)
	wp[:w.shape[0]] = w.detach()
	return wp


def _fold2_split_fresh(ops, w):
	wf = ops.fold2_pack_weight(w, torch.float32, 1)
	return ops.pack_weight_split3(wf.permute(1, 2, 0), BF16, want_dgrad = False)[:1]


# kind -> (parameter shape, request(W, _lib, w) -> tensors, fresh(ops, _lib, w) -> the same operands packed from scratch)
KINDS = {
	'packed_fwd': ((24, 16, 3), lambda W, L, w: (W.packed_weight(w, BF16, L.PACK_FWD), ), lambda ops, L, w: (ops.pack_weight(w, BF16, L.PACK_FWD), )),  # (cout_pad rounds 24 up: a forward copy of its own)
	'packed_dgrad': ((24, 16, 3), lambda W, L, w: (W.packed_weight(w, BF16, L.PACK_DGRAD), ), lambda ops, L, w: (ops.pack_weight(w, BF16, L.PACK_DGRAD), )),
	'packed_fwd_f32': ((24, 16, 3), lambda W, L, w: (W.packed_weight(w, torch.float32, L.PACK_FWD), ), lambda ops, L, w: (ops.pack_weight(w, torch.float32, L.PACK_FWD), )),
	'split_3_planes': ((64, 64, 3), lambda W, L, w: W.split_weight(w, BF16), lambda ops, L, w: ops.pack_weight_split3(w, BF16)),
	'split_1_plane': ((64, 64, 3), lambda W, L, w: W.split_weight(w, BF16, 1), lambda ops, L, w: ops.pack_weight_split3(w, BF16, dgrad_planes = 1)),
	'fold2_bf16': ((128, 64, 3), lambda W, L, w: (W.fold2_packed_weight(w, BF16, 1), ), lambda ops, L, w: (ops.fold2_pack_weight(w, BF16, 1), )),
	'fold2_split': ((128, 64, 3), lambda W, L, w: (W.fold2_split_weight(w, BF16, 1), ), lambda ops, L, w: _fold2_split_fresh(ops, w)),
	'head_dgrad_bf16': ((38, 128, 1), lambda W, L, w: (W.head_dgrad_weight(w, BF16), ), lambda ops, L, w: (ops.pack_weight(_padded_head(w), BF16, L.PACK_DGRAD), )),
	'head_split_3_planes': ((38, 128, 1), lambda W, L, w: W.head_split_weight(w, BF16), lambda ops, L, w: ops.pack_weight_split3(_padded_head(w), BF16)),
	'head_split_1_plane': ((38, 128, 1), lambda W, L, w: W.head_split_weight(w, BF16, 1), lambda ops, L, w: ops.pack_weight_split3(_padded_head(w), BF16, dgrad_planes = 1)),
}


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_every_kind_of_copy_follows_the_one_staleness_rule(kind):
	from convasr_amd import ops, _lib, weights as W
	shape, request, fresh = KINDS[kind]
	d = torch.device('cuda:0')
	torch.manual_seed(len(kind))
	w = torch.nn.Parameter(torch.randn(*shape, device = d))

	def asked(launches):
		"""One request: the operands and whether it cost C-ABI calls (launches: True -- at least one, False -- none)."""
		c0 = _lib.calls[0]
		got = request(W, _lib, w)
		assert (_lib.calls[0] > c0) == launches, (kind, _lib.calls[0] - c0)
		return got

	def same_buffers_fresh_values(got):
		assert [t.data_ptr() for t in got] == addresses
		want = fresh(ops, _lib, w)
		assert len(got) == len(want) and all(a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got, want)), kind

	first = asked(True)
	addresses = [t.data_ptr() for t in first]
	same_buffers_fresh_values(first)
	# 1. the parameter unchanged: the same tensor objects, no call
	again = asked(False)
	assert len(again) == len(first) and all(a is b for a, b in zip(again, first))
	# 2. an in-place update moves torch's version counter; an update behind torch's back counts once the epoch is bumped
	with torch.no_grad():
		w.add_(1)
	same_buffers_fresh_values(asked(True))
	w.data.mul_(0.5)
	asked(False)
	W.bump_param_epoch()
	same_buffers_fresh_values(asked(True))
	# 3. declared stale: packed again, into the same buffers, once
	W.force_repack()
	same_buffers_fresh_values(asked(True))
	asked(False)
	# 4. dropped: the structure epoch moves on and nothing holds the parameter any more
	epoch = W.structure_epoch()
	W.invalidate_pack_cache()
	assert W.structure_epoch() > epoch
	ref = weakref.ref(w)
	del w, first, again
	gc.collect()
	assert ref() is None, kind


def test_the_arena_mirror_serves_as_the_forward_copy_once_it_is_vouched_for():
	"""A tap-major arena weight whose Cout needs no padding has no bf16 forward copy of its own: the request returns the parameter's
	segment of flat.data16 -- packed into by a launch as long as nobody vouches for it, returned as it is after a fused optimizer step
	wrote it.  A mirror re-allocated in the other 16-bit type is zero-filled and vouched for by nobody: the next request packs it."""
	import convasr_amd as ca
	from convasr_amd import ops, _lib, weights as W
	d = torch.device('cuda:0')
	torch.manual_seed(0)
	model = torch.nn.Sequential(torch.nn.Conv1d(64, 128, 3), torch.nn.Conv1d(128, 64, 1)).to(d)
	flat = ca.train.FlatParameters(model)
	w = model[0].weight
	assert ops.weight_layout(w) == _lib.W_KMAJOR and ops.cout_pad(128) == 128

	def asked(dt, launches):
		c0 = _lib.calls[0]
		got = W.packed_weight(w, dt, _lib.PACK_FWD)
		assert _lib.calls[0] - c0 == launches
		lo = flat.data16.data_ptr()
		assert flat.data16.dtype == dt and got.dtype == dt and lo <= got.data_ptr() and got.data_ptr() + 2 * got.numel() <= lo + 2 * flat.numel  # a view into the mirror
		assert torch.equal(got, ops.pack_weight(w, dt, _lib.PACK_FWD))
		return got

	asked(BF16, 1)  # nobody has vouched for the segment yet: one packing launch, into the mirror
	asked(BF16, 0)
	opt = ca.train.SGD(flat, lr = 1e-1, momentum = 0.9, weight_decay = 1e-3)
	flat.grad.normal_()
	for p in flat.params:
		p._convasr_fresh = False  # (as after a backward pass: the gradients count)
	before = w.detach().clone()
	opt.step()
	assert not torch.equal(w.detach(), before)
	asked(BF16, 0)  # the optimizer kernel rewrote the segment with the parameters: carried over, no launch
	with torch.no_grad():
		w.mul_(2)  # changed by something that does not write the mirror: packed again
	asked(BF16, 1)
	flat.mirror(torch.float16)
	assert not bool(flat.data16.any())
	got = asked(torch.float16, 1)
	assert bool(got.any())
	flat.mirror(BF16)  # and back: the bf16 entry of before the switch pointed into a buffer that is gone, its version must not vouch for the new one
	got = asked(BF16, 1)
	assert bool(got.any())
