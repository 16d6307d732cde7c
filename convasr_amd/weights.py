"""Derived copies of parameters and the one rule for when they are stale.

Parameters keep the reference's fp32 (Cout, Cin, K) layout.  What the kernels consume -- packed 16-bit / fp32 operands, split-operand planes,
the folded prologue, the padded head -- are copies made by a packing launch, kept in ONE registry and refreshed, in place, only when the
parameter changed (param_version).  Every kind of copy goes through the same lookup (_current), so "declare everything stale"
(force_repack) and "drop everything" (invalidate_pack_cache) are one loop each and a new kind cannot be forgotten by either.

Also here, because they are the same bookkeeping: the dgrad pre-pack of a training step (prepack_dgrad_weights) and the validity of the
segments of train.FlatParameters' 16-bit mirror, which serve as packed forward copies that the fused optimizer kernels keep current."""
import os

import torch

from . import ops, _lib

_param_epoch = [0]  # bumped by optimizers that update parameters behind torch's back (convasr_amd.train.SGD)
_structure_epoch = [0]
_entries = {}  # (id(parameter), kind, what the kind is made for ...) -> dict(w = the parameter, ver = the version `out` is current for, out = the copy, ...)
HEAD_PAD = 128  # channels the gradient of a narrow 1x1 head is padded to in backward


def bump_param_epoch():
	_param_epoch[0] += 1


def param_version(w):
	"""What a packed copy of `w` is valid for: torch's in-place version counter, the storage address, and the epoch optimizers bump
	when they update parameters behind torch's back."""
	return (w._version, w.data_ptr(), _param_epoch[0])


def structure_epoch():
	return _structure_epoch[0]


def _entry(w, key):
	ent = _entries.get((id(w), ) + key)
	if ent is None:
		ent = _entries[(id(w), ) + key] = dict(w = w, ver = None, out = None)  # holds `w`: id() stays unique
	return ent


def _current(w, key, refresh, *args):
	"""The registry's one lookup: the copy of `w` of kind `key`, made on first use and refreshed by refresh(ent, w, ver, *args) when the
	parameter's version is not the one the entry was made for.  A refresh writes into the buffers of the earlier call (ent['out']): captured
	step graphs bake their addresses."""
	ver = param_version(w)
	ent = _entry(w, key)
	if ent['ver'] != ver:
		refresh(ent, w, ver, *args)
		ent['ver'] = ver
	return ent['out']


def force_repack():
	"""Declare every copy that a launch of this module keeps current stale (the arena's 16-bit mirror segments, which the fused
	optimizer kernels write, stay vouched for): the next forward / backward re-packs them all.  train.GraphedTrainStep calls it right
	before a capture so that the graph records every per-step pack launch whatever ran since the last optimizer step."""
	for ent in _entries.values():
		if ent.get('flat') is None:
			ent['ver'] = None


def invalidate_pack_cache():
	"""Called when conv modules were replaced (fuse_conv_bn_eval): every copy is dropped -- with it the reference to its parameter -- and
	everything derived from the module tree (JasperNet's list of dgrad weights, captured step graphs) is rebuilt on next use."""
	_entries.clear()
	_structure_epoch[0] += 1


# ------------------------------------------------------------------------------------------------ the arena's 16-bit mirror

def mirror_reallocated(flat):
	"""flat.data16 is a new, zero-filled buffer (FlatParameters.mirror in the other 16-bit type) or does not exist yet (a new
	FlatParameters): no segment is vouched for, and an entry left from before the switch must not serve the old buffer.
	flat.mirror_vouchers: id(param) -> version at which the parameter's segment of flat.data16 equals the parameter rounded to 16 bits."""
	flat.mirror_vouchers = {}
	for ent in _entries.values():
		if ent.get('flat') is flat:
			ent['ver'] = None


def mirror_carried_over(flat, run):
	"""Run one fused optimizer launch `run(p16)` that rewrites the 16-bit mirror together with the parameters (or leaves both
	untouched when the device-side gate skips the step): segments that were current before it are current after it."""
	vouched = flat.mirror_vouchers
	was = [k for k, v in vouched.items() if v == param_version(flat._by_id[k])]
	run(flat.data16)
	bump_param_epoch()  # packed compute copies other than the mirror are stale now
	vouched.clear()
	if flat.data16 is not None:
		for k in was:
			vouched[k] = param_version(flat._by_id[k])


# ------------------------------------------------------------------------------------------------ packed forward / dgrad operands

def _arena_segment(w, dtype):
	"""(flat, offset) when the arena itself holds the packed forward operand of `w`: a tap-major arena parameter (train.FlatParameters)
	whose Cout needs no row padding.  In fp32 the master IS the packed operand, in bf16 / fp16 it is the parameter's segment of the arena's
	16-bit mirror."""
	arena = getattr(w, '_convasr_arena', None)
	# (the address test: p.data may have been replaced since FlatParameters re-homed it -- model.to(), load_state_dict(assign = True) --
	# with the strides preserved; such a parameter no longer aliases the arena and is packed like any other)
	in_place = arena is not None and (ops.weight_layout(w) == _lib.W_KMAJOR or (w.shape[2] == 1 and w.is_contiguous())) and ops.cout_pad(w.shape[0]) == w.shape[0] and dtype in (torch.float32, ) + ops.HALF_DTYPES and w.device == arena[0].data.device and w.data_ptr() == arena[0].data.data_ptr() + 4 * arena[1]
	return arena if in_place else None


def _serve_from_arena(fwd, w, ver, dtype):
	"""Point the forward entry at the arena when it holds the operand (_arena_segment).  Returns (is the copy current without a launch?,
	the arena whose mirror a packing launch into fwd['out'] makes current -- to be vouched for -- or None)."""
	arena = _arena_segment(w, dtype)
	if arena is None:
		if fwd.pop('in_arena', False):  # it was served from the arena until p.data was replaced: from here on a copy of its own, declared stale like any other
			fwd['out'] = None
			fwd.pop('flat', None)
			return False, None
		return fwd['ver'] == ver, None
	flat, off = arena
	Cout, Cin, K = w.shape
	fwd['in_arena'] = True
	if dtype == torch.float32:
		fwd['out'] = flat.data[off:off + w.numel()].view(K, Cout, Cin)
		return True, None
	# the mirror segment is current only if the arena says so for THIS version: a mirror re-allocated in the other 16-bit type
	# (FlatParameters.mirror) is zero-filled, and a cache entry left from before the switch must not vouch for it
	fwd['out'] = flat.mirror(dtype)[off:off + w.numel()].view(K, Cout, Cin)
	fwd['flat'] = flat  # (what force_repack leaves alone and mirror_reallocated looks for)
	return flat.mirror_vouchers.get(id(w)) == ver, flat


def _refresh_fwd(fwd, w, ver, dtype):
	"""The forward copy alone, also in training: the dgrad copies of a step are made together, by prepack_dgrad_weights' one launch."""
	current, flat = _serve_from_arena(fwd, w, ver, dtype)
	if not current:
		fwd['out'] = ops.pack_weight(w, dtype, _lib.PACK_FWD, out = (fwd['out'], None))
		if flat is not None:
			flat.mirror_vouchers[id(w)] = ver


def _refresh_dgrad(dgr, w, ver, dtype):
	"""The forward and the dgrad layout in one launch (the forward half is skipped when the arena's mirror already holds it)."""
	fwd = _entry(w, ('fwd', dtype))
	current, flat = _serve_from_arena(fwd, w, ver, dtype)
	fwd['out'], dgr['out'] = ops.pack_weight(w, dtype, None, out = (fwd['out'], dgr['out']), fwd_is_current = current)
	fwd['ver'] = ver
	if flat is not None:
		flat.mirror_vouchers[id(w)] = ver


def packed_weight(w, dtype, mode):
	"""Packed [K][rows_pad][cols] copy of a conv parameter, refreshed (in place) only when the parameter changed.  The forward and the
	dgrad copy keep separate versions: a dgrad request refreshes both in one launch, a forward request the forward copy alone.
	A tap-major arena parameter (train.FlatParameters) whose Cout needs no row padding has no forward copy of its own: in fp32
	the master IS the packed operand, in bf16 / fp16 it is the parameter's segment of the arena's 16-bit mirror, which the fused optimizer
	kernels keep current -- only the transposed dgrad copy is still built by a packing launch."""
	if mode == _lib.PACK_DGRAD:
		return _current(w, ('dgr', dtype), _refresh_dgrad, dtype)
	return _current(w, ('fwd', dtype), _refresh_fwd, dtype)


# ------------------------------------------------------------------------------------------------ split-operand planes

def _refresh_split(ent, w, ver, dtype, dgrad_planes):
	ent['out'] = ops.pack_weight_split3(w, dtype, out = ent['out'], dgrad_planes = dgrad_planes)


def split_weight(w, dtype, dgrad_planes = 3):
	"""(forward, dgrad) split operands of a conv parameter for the split-operand path (csrc/split3.hip): hi / lo planes of the fp32 master
	in the 16-bit type `dtype`, both refreshed by ONE launch when the parameter changed (in place: stable addresses).  dgrad_planes = 1: the
	dgrad operand is the ordinary 16-bit one (w_hi alone), for layers whose backward runs one product per gradient (cfg['split_hi_bwd'])."""
	return _current(w, ('split', dtype, dgrad_planes), _refresh_split, dtype, dgrad_planes)


# ------------------------------------------------------------------------------------------------ the folded stride-2 prologue (functional.Fold2)

def _refresh_fold2(ent, w, ver, dt, pad):
	ent['out'] = ops.fold2_pack_weight(w, dt, pad, out = ent['out'])


def fold2_packed_weight(weight, dt, pad):
	"""Packed forward operand [K'][cout_pad][2 Cin] of the folded conv."""
	return _current(weight, ('fold2', dt), _refresh_fold2, dt, pad)


def _refresh_fold2_split(ent, w, ver, split, pad):
	ent['wf'] = ops.fold2_pack_weight(w, torch.float32, pad, out = ent.get('wf'))  # [K'][Cout][2 Cin] fp32 (Cout % 128 == 0: no padded rows)
	ent['out'] = ops.pack_weight_split3(ent['wf'].permute(1, 2, 0), split, out = (ent['out'], None), want_dgrad = False)[0]


def fold2_split_weight(weight, split, pad):
	"""Forward planes [K'][Cout][3 x 2 Cin] of the folded conv of a split-operand network: the fp32 folded weight (convasr_fold2_pack_weight
	into a tap-major fp32 buffer) split like any other (split_weight's kernel); refreshed per parameter version, in place."""
	return _current(weight, ('fold2', 'split', split), _refresh_fold2_split, split, pad)


# ------------------------------------------------------------------------------------------------ the narrow head as a 128-class problem (functional._HeadPad)

def _refresh_head_dgrad(ent, w, ver, dt):
	Cout, Cin, K = w.shape
	if ent['out'] is None:
		ent['out'] = torch.zeros(1, ops.cout_pad(Cin), HEAD_PAD, dtype = dt, device = w.device)
	src = w.detach()
	# wd[0][ci][co] = w[co][ci][0]: the layout kernel reads (C = co, T = ci) and writes it channels-last with a row pitch of 128
	_lib.call('convasr_convert_layout', _lib.ptr(src), _lib.F32, 0, src.stride(0), src.stride(1), _lib.ptr(ent['out']), _lib.dtype_code(dt), 0, 1, HEAD_PAD, 1, Cout, Cin, _lib.stream_ptr())


def head_dgrad_weight(weight, dt):
	"""The head's weight transposed into a zero-padded [Cin][128] dgrad operand."""
	return _current(weight, ('head', dt), _refresh_head_dgrad, dt)


def _refresh_head_split(ent, w, ver, split, dgrad_planes):
	Cout, Cin, K = w.shape
	if ent['out'] is None:
		ent['wp'], ent['out'] = torch.zeros(HEAD_PAD, Cin, 1, dtype = torch.float32, device = w.device), (None, None)
	src, wp = w.detach(), ent['wp']
	_lib.call('convasr_convert_layout', _lib.ptr(src), _lib.F32, 0, src.stride(0), src.stride(1), _lib.ptr(wp), _lib.F32, 0, wp.stride(0), wp.stride(1), 1, Cout, Cin, _lib.stream_ptr())
	ent['out'] = ops.pack_weight_split3(wp, split, out = ent['out'], dgrad_planes = dgrad_planes)


def head_split_weight(weight, split, dgrad_planes = 3):
	"""(forward, dgrad) planes of a narrow one-tap head in a split-operand network, as 128-class operands: the fp32 weight is copied into the
	live rows of a zero-padded (128, Cin, 1) fp32 buffer and split like any other weight; refreshed per parameter version, in place.
	dgrad_planes = 1: the dgrad operand as the ordinary 16-bit one (a one-product backward, split_weight)."""
	return _current(weight, ('head', 'split', split, dgrad_planes), _refresh_head_split, split, dgrad_planes)


# ------------------------------------------------------------------------------------------------ the dgrad pre-pack of a training step

# The transposed, tap-flipped dgrad copies of the weights (one ~8 us memory-bound launch per layer and step) depend on nothing but the
# parameters, and the step has one stretch where most of the chip idles: the CTC alpha / beta recursion, one workgroup per utterance
# (64 of 256 CUs, ~0.3 ms of dependent steps).  prepack_dgrad_weights() -- called by the network between the decoder and the loss --
# runs those launches on a side stream there; the first dgrad of the backward pass joins it (join_prepack).
PREPACK = os.environ.get('CONVASR_NO_PREPACK') != '1'  # A/B hook
GRAPHS_CAPTURED = [False]  # set by train.GraphedTrainStep at its first capture: from then on an eager step (the warm-up of a new batch shape, a shape beyond max_graphs) makes its dgrad copies on the MAIN stream -- see prepack_dgrad_weights
_prepack_streams = {}  # device -> [side stream, packs pending on it?]


GROUPED_PACK_MIN = int(os.environ.get('CONVASR_GROUPED_PACK_MIN', 32))
_pack_tables = {}  # (device, dtype, the (src, dst) addresses of the group) -> dict(items = device table, blocks, n); entries live as long as the process: graphs bake their addresses


def _pack_group(stale, dtype, refresh = True):
	"""Which of the `stale` weights' dgrad copies can share the one grouped launch: 16-bit, even channel counts, buffers allocated, packed
	forward copy current (the arena mirror's segment, or refreshed here when refresh is set)."""
	group = []
	# (a grouped launch only for MANY copies: the one launch floods every CU at once -- beside the CTC recursion, whose 64 polling workgroups
	# it overlaps on the prepack stream, that cost the Wav2Letter step +40 us of CTC time for 18 copies, where 18 small launches cost nothing;
	# JasperNetLarge's 108 copies drop from 0.83 to 0.24 ms: profiles/r05_ab_rounds_wav2letter.json, r05_config4_kernel_stats.csv)
	if dtype in ops.HALF_DTYPES and len(stale) >= GROUPED_PACK_MIN:
		for w in stale:
			dgr = _entries.get((id(w), 'dgr', dtype))
			if dgr is None or dgr['out'] is None:
				continue
			fwd = packed_weight(w, dtype, _lib.PACK_FWD) if refresh else _entries[(id(w), 'fwd', dtype)]['out']  # (no launch when the optimizer's 16-bit mirror serves it)
			Cout, Cin, K = w.shape
			if fwd is not None and Cout % 2 == 0 and Cin % 2 == 0 and fwd.dtype == dtype:
				group.append((w, dgr, fwd))
	return group


def _pack_table(group, dtype):
	"""The device-resident item table of a group (rebuilt -- one small host-to-device copy -- only when the set of buffers changed)."""
	import struct
	dev = group[0][0].device
	key = tuple((fwd.data_ptr(), dgr['out'].data_ptr()) for _, dgr, fwd in group)
	tab = _pack_tables.get((dev, dtype, key))  # one table per set of buffers, never dropped: a captured step graph holds its address (a few KB each)
	if tab is None:
		if ops._capturing[0]:
			raise _lib.ConvasrHipError('the dgrad pack table changed while a step graph is being captured (GraphedTrainStep prewarms it: weights.prewarm_dgrad_pack)')
		assert _lib.load().convasr_pack_dgrad_item_bytes() == 40
		blob, first = b'', 0
		for w, dgr, fwd in group:
			Cout, Cin, K = w.shape
			blob += struct.pack('<QQiiiiii', fwd.data_ptr(), dgr['out'].data_ptr(), Cout, Cin, K, ops.cout_pad(Cout), ops.cout_pad(Cin), first)
			first += K * ((Cout + 63) // 64) * ((Cin + 63) // 64)
		tab = _pack_tables[(dev, dtype, key)] = dict(key = key, items = torch.frombuffer(bytearray(blob), dtype = torch.uint8).to(dev), blocks = first, n = len(group))
	return tab


def prewarm_dgrad_pack(weights, dtype):
	"""Build the grouped pack's device table for the weights a training step will re-pack (all of them: every optimizer step makes every
	copy stale), outside a graph capture -- the capture itself cannot copy a table to the device."""
	group = _pack_group([w for w in weights], dtype, refresh = False)
	if group:
		_pack_table(group, dtype)


def _pack_dgrad_many(stale, dtype):
	"""The transposed dgrad copies of the `stale` weights: ONE launch for all those whose packed forward copy is current and 16-bit (the
	arena mirror's segments, or a forward pack refreshed here), a launch each for the rest."""
	group = _pack_group(stale, dtype)
	grouped = {id(w) for w, _, _ in group}
	for w in stale:
		if id(w) not in grouped:
			packed_weight(w, dtype, _lib.PACK_DGRAD)
	if not group:
		return
	tab = _pack_table(group, dtype)
	_lib.call('convasr_pack_dgrad_grouped', _lib.ptr(tab['items']), tab['n'], tab['blocks'], _lib.stream_ptr())
	for w, dgr, _ in group:
		dgr['ver'] = param_version(w)


def prepack_dgrad_weights(weights, dtype):
	if not weights:
		return
	dev = weights[0].device
	join_prepack(dev)  # (a previous step that never reached its backward pass -- a loss skipped on the host -- left its packs unjoined)
	stale = []
	for w in weights:
		dgr = _entries.get((id(w), 'dgr', dtype))
		if dgr is None or dgr['out'] is None:
			packed_weight(w, dtype, _lib.PACK_DGRAD)  # first use: buffers are allocated (and stay owned) by the main stream
		elif dgr['ver'] != param_version(w):
			stale.append(w)
	if not stale:
		return
	# Once step graphs exist in this process, eager steps stay off the prepack stream too: one stream less at the boundary between an eagerly
	# launched step and a replayed one, where round 6 found a race (profiles/r06_interleave_race.txt).  This alone did not close it -- what does
	# is the host wait per transition in train.GraphedTrainStep._fence_transition -- but it removed the variant in which the replayed step's
	# pack nodes rewrote buffers an eager step had just packed on the side stream (scratch/r6_interleave_debug2.py: differing losses in every other
	# run before, none in 8 after).  Eager steps are the exception once graphs exist, so they simply do not fork.
	if not PREPACK or GRAPHS_CAPTURED[0]:  # (A/B hook, and what a linear step-graph capture sets: the copies are made on the main stream, still in one launch)
		_pack_dgrad_many(stale, dtype)
		return
	st = _prepack_streams.get(dev)
	if st is None:
		st = _prepack_streams[dev] = [torch.cuda.Stream(device = dev), False]
	side, main = st[0], torch.cuda.current_stream(dev)
	_lib.stream_wait(side, main)  # the parameters, their 16-bit mirror and every earlier reader of the buffers are ordered before the packs
	with torch.cuda.stream(side):
		_pack_dgrad_many(stale, dtype)
	st[1] = True


def join_prepack(device):
	st = _prepack_streams.get(device)
	if st is not None and st[1]:
		_lib.stream_wait(torch.cuda.current_stream(device), st[0])
		st[1] = False
