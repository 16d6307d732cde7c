"""Training-step plumbing for the hot path (reference: train.py:745-783).

FlatParameters re-homes every trainable parameter into ONE contiguous fp32 buffer with a matching gradient buffer, so that
gradient clipping is one reduction launch, the optimizer one elementwise launch, and data-parallel all-reduce a handful of
large contiguous RCCL calls (288 GB of HBM makes the duplicate-free arena trivially affordable).  Backward kernels write
gradients straight into the arena (convasr_amd.functional._deliver_many).

Conv weights live in the arena TAP-MAJOR ([K][Cout][Cin], include/convasr_hip.h CONVASR_W_KMAJOR): the parameter stays a
(Cout, Cin, K) tensor -- state_dict(), load_state_dict() and checkpoints see the reference's shapes -- but it is a strided view.
That is the element order of the packed MFMA operand and of the weight-gradient slabs, so (a) the optimizer kernel also writes a
bf16 mirror of the arena whose conv segments ARE the packed forward weights (no packing launches per step), and (b) the split-K
combine of the weight gradient is a streaming sum instead of a transpose."""
import contextlib
import math
import os

import torch

from . import ops, _lib
from . import models as M
from . import functional as Fn
from . import weights as W
from .optimizers import _advance


class FlatParameters:
	ALIGN = 64  # elements: every parameter starts on a 256-byte boundary

	def __init__(self, model):
		params = [p for p in model.parameters() if p.requires_grad]
		if not params:
			raise ValueError('model has no trainable parameters')
		dev = params[0].device
		self.params, self.offsets = params, []
		off = 0
		for p in params:
			if p.dtype != torch.float32 or p.device != dev:
				raise ValueError('FlatParameters needs fp32 parameters on one device')
			self.offsets.append(off)
			off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
		self.numel = off
		self.data = torch.zeros(off, dtype = torch.float32, device = dev)
		self.grad = torch.zeros(off, dtype = torch.float32, device = dev)
		W.mirror_reallocated(self)  # (no mirror yet: nothing is vouched for)
		self.data16 = None  # 16-bit (bf16 or fp16: the model's compute dtype) mirror of `data`, allocated on first use (mirror()); written by the fused optimizer kernels
		self._as_param = []  # per parameter: flat arena-shaped tensor -> view in the parameter's logical (reference) shape
		for p, o in zip(params, self.offsets):
			n = p.numel()
			kmajor = p.ndim == 3 and p.shape[2] > 1 and (p.shape[0] * p.shape[1]) % 8 == 0 and dev.type == 'cuda'
			as_param = (lambda flat, p = p, o = o, n = n: flat[o:o + n].view(p.shape[2], p.shape[0], p.shape[1]).permute(1, 2, 0)) if kmajor else (lambda flat, p = p, o = o, n = n: flat[o:o + n].view(p.shape))  # (o, n bound now: the views are rebuilt later for optimizer state)
			self._as_param.append(as_param)
			view = as_param(self.data)
			view.copy_(p.data)
			p.data = view
			p._convasr_grad = as_param(self.grad)
			p._convasr_fresh = True
			# (a one-tap conv weight, (Cout, Cin, 1) contiguous, IS its own tap-major form: its mirror segment serves as the packed forward
			# operand just the same -- the dense-residual models carry ~55 such 1x1 convs, one packing launch each per step otherwise)
			one_tap = p.ndim == 3 and p.shape[2] == 1 and (p.shape[0] * p.shape[1]) % 8 == 0 and dev.type == 'cuda'
			p._convasr_arena = (self, o) if (kmajor or one_tap) else None
			p.grad = p._convasr_grad
		self._by_id = {id(p): p for p in params}
		self.clip = None  # (sumsq double buffer, max_norm) set by clip_grad_norm_
		self.grad_scale = 1.0  # pending scale of .grad (the data-parallel engine's 1 / world_size), consumed by the next optimizer step
		self._sumsq = torch.zeros(1, dtype = torch.float64, device = dev)
		self.loss_scaler = None  # a LossScaler (fp16 training): .grad then holds gradients of the SCALED loss until the optimizer step unscales them
		self.averaged = None  # the WeightEMA whose average_parameters() context is open: the arena then holds the AVERAGE, and nothing may step it

	def mirror(self, dtype = torch.bfloat16):
		"""The arena's 16-bit mirror in `dtype` (one at a time: asking for the other type re-allocates it and drops what was current)."""
		if self.data16 is None or self.data16.dtype != dtype:
			assert dtype in ops.HALF_DTYPES
			self.data16 = torch.zeros(self.numel, dtype = dtype, device = self.data.device)
			W.mirror_reallocated(self)
		return self.data16

	def mirror_carried_over(self, run):
		"""Run one fused optimizer launch `run(p16)` that rewrites the 16-bit mirror together with the parameters (or leaves both
		untouched when the device-side gate skips the step): segments that were current before it are current after it."""
		if self.averaged is not None:
			raise _lib.ConvasrHipError('the arena holds the averaged weights (inside WeightEMA.average_parameters()): no optimizer step, step-graph replay or copy_to until the context is left')
		W.mirror_carried_over(self, run)

	def param_views(self, flat_tensor):
		"""Per-parameter views of an arena-shaped tensor (optimizer state) in the parameters' logical shapes -- the reference's
		(Cout, Cin, K) for conv weights, whatever the arena's element order is."""
		assert flat_tensor.numel() == self.numel
		return [f(flat_tensor) for f in self._as_param]

	def export_state(self, flat_tensor):
		"""Arena-shaped optimizer state -> list of contiguous per-parameter tensors in reference shapes (layout-independent checkpoints)."""
		return [v.contiguous().clone() for v in self.param_views(flat_tensor)]

	def import_state(self, flat_tensor, per_param, what):
		if isinstance(per_param, torch.Tensor):
			raise ValueError(f'{what}: a flat arena-ordered tensor (optimizer state written before format 2) carries no layout tag and cannot be loaded safely: conv segments may be tap-major or reference-ordered')
		views = self.param_views(flat_tensor)
		if len(per_param) != len(views):
			raise ValueError(f'{what}: {len(per_param)} tensors for {len(views)} parameters')
		for v, t in zip(views, per_param):
			if tuple(v.shape) != tuple(t.shape):
				raise ValueError(f'{what}: shape {tuple(t.shape)} does not match parameter shape {tuple(v.shape)}')
			v.copy_(t)

	def zero_grad(self):
		"""No memset: the next backward overwrites (first write per parameter has accumulate = False)."""
		for p in self.params:
			p._convasr_fresh = True
			p.grad = p._convasr_grad
		self.clip = None

	def grads_written_externally(self):
		"""Call after anything other than this package's backward kernels wrote into `.grad` / `p._convasr_grad` (an optimizer that keeps its
		clipped gradients there, a test, a hand-rolled gradient edit): drops the "this segment is known to be zero" notes the train-mode
		residual branches keep for their conv biases (functional.ConvBnActFunction), so that the next backward zeroes them again."""
		for p in self.params:
			if getattr(p, '_convasr_grad_is_zero', False):
				p._convasr_grad_is_zero = False

	def finalize_grads(self):
		"""Parameters that received no gradient this step count as zero."""
		for p in self.params:
			if p._convasr_fresh:
				p._convasr_grad.zero_()

	def clip_grad_norm_(self, max_norm):
		"""torch.nn.utils.clip_grad_norm_(params, max_norm) (train.py:777): one reduction launch now; the scaling itself is
		folded into the optimizer kernel.  Returns the total norm as a 0-d device tensor (no host sync)."""
		self.finalize_grads()
		norm = torch.empty(1, dtype = torch.float32, device = self.grad.device)
		ops.sumsq(self.grad, self._sumsq, norm_out = norm, norm_scale = self.grad_scale, loss_scaler = None if self.loss_scaler is None else self.loss_scaler.current)
		self.clip = (self._sumsq, float(max_norm))
		return norm[0]


class LossScaler:
	"""Dynamic loss scaling for fp16 training: the role apex.amp's LossScaler plays behind `apex.amp.initialize(opt_level)`
	(models.py:744-762) and `with apex.amp.scale_loss(loss, optimizer)` (train.py:770-772), with apex's defaults (initial scale 2^16,
	x 2 after 2000 clean steps, / 2 and the step skipped on overflow, ceiling 2^24).  The state lives on the device
	(include/convasr_hip.h, CONVASR_LOSS_SCALER_FLOATS) in two buffers: every optimizer step reads `current` and writes the other one,
	advance() swaps them -- the host never waits for the overflow verdict.  loss_scale = a number: static scale (apex's
	loss_scale = 128.0 form), no overflow check."""

	def __init__(self, device, loss_scale = 'dynamic', init_scale = 2.0 ** 16, scale_factor = 2.0, scale_window = 2000, min_loss_scale = None, max_loss_scale = 2.0 ** 24):
		dynamic = loss_scale in (None, 'dynamic')
		state = [float(init_scale) if dynamic else float(loss_scale), 0.0, 0.0, float(scale_window) if dynamic else 0.0, float(min_loss_scale or 0.0), float(max_loss_scale), float(scale_factor), 0.0]
		assert len(state) == _lib.LOSS_SCALER_FLOATS
		self.state = torch.tensor([state, state], dtype = torch.float32, device = device)
		self.cur = 0
		self.pinned = False  # set by the first step-graph capture: from then on the current row stays where the graphs read it (see advance)

	@property
	def current(self):
		return self.state[self.cur]

	def pair(self):
		return self.state[self.cur], self.state[1 - self.cur]

	def advance(self):
		"""After an optimizer launch wrote the next state into the other buffer: swap the two -- or, once a step graph has been captured
		(its kernels read THIS buffer at every replay; `pinned`, eager steps included: optimizers._advance), enqueue the copy that hands the
		new state back to it."""
		if Fn.capturing() or self.pinned:
			_lib.call('convasr_copy', _lib.ptr(self.state[1 - self.cur]), _lib.ptr(self.state[self.cur]), 4 * _lib.LOSS_SCALER_FLOATS, _lib.stream_ptr())
		else:
			self.cur = 1 - self.cur

	def loss_scale(self):
		"""Host read (synchronises): apex's `_amp_state.loss_scalers[0].loss_scale()`."""
		return float(self.current[0])

	def state_dict(self):
		"""apex.amp.state_dict()'s entry for one scaler (train.py:332 saves it as `amp_state_dict`)."""
		s = self.current.tolist()
		return dict(loss_scale = s[0], unskipped = int(s[1]))

	def load_state_dict(self, sd):
		cur = self.current.clone()
		cur[0], cur[1] = float(sd['loss_scale']), float(sd['unskipped'])
		self.state[self.cur].copy_(cur)


def amp_state_dict(optimizer):
	"""apex.amp.state_dict() (train.py:332): {'loss_scaler0': {...}} when the optimizer trains under a loss scaler, else {}."""
	scaler = getattr(getattr(optimizer, 'flat', None), 'loss_scaler', None)
	return {} if scaler is None else dict(loss_scaler0 = scaler.state_dict())


def amp_load_state_dict(optimizer, sd):
	"""apex.amp.load_state_dict(checkpoint['amp_state_dict']) (train.py:707-708)."""
	scaler = getattr(getattr(optimizer, 'flat', None), 'loss_scaler', None)
	if scaler is not None and sd and 'loss_scaler0' in sd:
		scaler.load_state_dict(sd['loss_scaler0'])


class SGD:
	"""torch.optim.SGD semantics (train.py:657-662) as ONE fused kernel launch over the flat arena."""

	def __init__(self, flat: FlatParameters, lr = 1e-2, momentum = 0.9, weight_decay = 1e-3, nesterov = False, keep_clipped_grads = False):
		self.flat = flat
		self.param_groups = [dict(params = flat.params, lr = lr, momentum = momentum, weight_decay = weight_decay, nesterov = nesterov)]
		self.momentum_buffer = torch.zeros_like(flat.data) if momentum != 0 else None
		self.steps = 0
		self.keep_clipped_grads = keep_clipped_grads
		self.lr_dev = None  # 1-element fp32 device tensor the captured step graphs read the learning rate from (GraphedTrainStep keeps it equal to param_groups[0]['lr'])

	def zero_grad(self, set_to_none = False):
		self.flat.zero_grad()

	def step(self, loss_gate = None):
		"""loss_gate: optional 1-element fp32 device tensor; a non-finite value turns the launch into a no-op (device-side skip)."""
		g = self.param_groups[0]
		flat = self.flat
		if flat.clip is None:
			flat.finalize_grads()
		sumsq, max_norm = flat.clip if flat.clip is not None else (None, 0.0)
		first, grad_scale = self.steps == 0, flat.grad_scale
		if first and Fn.capturing():
			raise _lib.ConvasrHipError('SGD: the first step (which initialises the momentum buffer) cannot be the one captured into a step graph')
		scaler = flat.loss_scaler
		if scaler is not None and sumsq is None:  # the overflow check reads the gradient's sum of squares
			sumsq = ops.sumsq(flat.grad, flat._sumsq)
		flat.mirror_carried_over(lambda p16: ops.sgd_step(flat.data, flat.grad, self.momentum_buffer, flat.numel, sumsq, max_norm, g['lr'], g['momentum'], g['weight_decay'], g['nesterov'], first, grad_out = flat.grad if self.keep_clipped_grads else None, loss_gate = loss_gate, grad_scale = grad_scale, p16 = p16, scaler = None if scaler is None else scaler.pair(), lr_dev = self.lr_dev if Fn.capturing() else None))
		if scaler is not None:
			scaler.advance()
		if self.keep_clipped_grads:
			flat.grads_written_externally()  # (zero times a NaN clip factor is not zero)
		self.steps += 1
		flat.clip, flat.grad_scale = None, 1.0

	def state_dict(self):
		"""format 2: momentum per parameter, in the reference's shapes (independent of the arena's tap-major element order)."""
		return dict(format = 2, steps = self.steps, momentum_buffer = None if self.momentum_buffer is None else self.flat.export_state(self.momentum_buffer), param_groups = [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups])

	def load_state_dict(self, sd):
		self.steps = sd['steps']
		if self.momentum_buffer is not None and sd.get('momentum_buffer') is not None:
			self.flat.import_state(self.momentum_buffer, sd['momentum_buffer'], 'SGD.load_state_dict(momentum_buffer)')
		for g, s in zip(self.param_groups, sd['param_groups']):
			g.update(s)


class WeightEMA:
	"""An exponential moving average of every trainable parameter, kept on the device as a second arena, for validation and for export.

	update() is ONE fused launch over the arena (convasr_ema_update): average += (1 - d) (w - average) with d = min(decay, (1 + k) / (10 + k)),
	k the number of updates applied so far -- a device counter, so a captured step graph replays the warm-up schedule; the first applied
	update copies the weights.  When the arena has a 16-bit mirror (flat.data16) the launch writes the average's mirror with it.  Call it
	after optimizer.step with the step's loss_gate (train_step(..., ema = ema) does): a step the optimizer skipped on the device -- a
	non-finite loss, or an overflow under flat.loss_scaler, whose verdict the kernel reads from the scaler's state -- leaves the average, its
	mirror and the counter untouched, without the host learning of it.

	average_parameters() EXCHANGES the contents of the arena and the average (and of the two mirrors), it does not re-point the parameters: the
	arena's address is baked into captured step graphs and keys every packed weight copy (weights.param_version).  Only parameters are
	averaged.  Buffers -- the batch-norm running statistics -- are not: inside the context the model runs the averaged parameters with its
	CURRENT running statistics.

	Data-parallel training needs nothing extra: every rank applies the same updates to equal weights, so the ranks hold equal averages."""

	def __init__(self, flat, decay = 0.999):
		if not 0.0 <= decay <= 1.0:
			raise ValueError(f'WeightEMA: decay {decay} is not in [0, 1]')
		self.flat, self.decay = flat, float(decay)
		self.average = flat.data.clone()  # (before the first update the average IS the weights; the first applied update overwrites it anyway)
		self.average16 = None  # 16-bit mirror of `average` in flat.data16's type: made by _mirror(), rewritten by every update
		self.count = torch.zeros(2, 1, dtype = torch.float32, device = flat.data.device)  # [_cur] is current: updates applied so far (the launch reads it and writes the other row)
		self._cur = 0
		self._pinned = False  # set by the first step-graph capture (pin): from then on the counter is handed back to the row the graphs read
		self._mirror()

	def _mirror(self):
		"""The average's mirror, following flat.data16: made from the average (round-to-nearest-even, what the kernel writes) when the arena
		has a mirror and this one is missing or of the other 16-bit type."""
		d16 = self.flat.data16
		if d16 is not None and (self.average16 is None or self.average16.dtype != d16.dtype):
			if Fn.capturing():
				raise _lib.ConvasrHipError('WeightEMA: the update that allocates the average\'s 16-bit mirror cannot be the one captured into a step graph')
			self.average16 = self.average.to(d16.dtype)
		return self.average16 if d16 is not None else None

	def pin(self):
		"""Called by GraphedTrainStep before a capture: the mirror exists, and the counter's current row stops moving."""
		self._mirror()
		self._pinned = True

	@property
	def updates(self):
		"""Updates applied so far (host read: synchronises)."""
		return int(self.count[self._cur, 0].item())

	def _refuse_inside(self, what):
		if self.flat.averaged is not None:
			raise _lib.ConvasrHipError(f'WeightEMA.{what}: the arena holds the averaged weights (inside average_parameters()); leave the context first')

	def update(self, loss_gate = None):
		"""One launch (plus, once a step graph has been captured, the one-float hand-back of the counter).  loss_gate: the 1-element gate the
		optimizer step was given, or None."""
		self._refuse_inside('update')
		flat, cur = self.flat, self._cur
		scaler = flat.loss_scaler
		ops.ema_update(flat.data, self.average, self.decay, self.count[cur], self.count[1 - cur], e16 = self._mirror(), loss_gate = loss_gate, scaler_state = None if scaler is None else scaler.current)
		_advance(self, self.count)

	def _exchange(self, d16, was):
		"""arena <-> average, and d16 <-> the average's mirror while d16 is still the arena's mirror.  Every packed copy goes stale (the epoch);
		the mirror segments `was` vouched for are vouched for again: each mirror was current for its own fp32 buffer and travels with it."""
		flat = self.flat
		ops.swap_(flat.data, self.average)
		W.bump_param_epoch()
		if flat.data16 is d16:
			if d16 is not None:
				ops.swap_(d16, self.average16)
			flat.mirror_vouchers = {k: W.param_version(flat._by_id[k]) for k in was} if d16 is not None else {}
		else:  # the arena's mirror was (re)allocated inside the context: it vouches for nothing, and the average's old mirror is of the wrong type
			W.mirror_reallocated(flat)
			self.average16 = None

	@contextlib.contextmanager
	def average_parameters(self):
		"""with ema.average_parameters(): the model's parameters ARE the average (two exchange launches on entry, two on exit, also when the body
		raises); buffers stay the model's own.  Packed weight copies made from the raw weights are not served for the averaged ones, or the
		reverse; mirror segments that were current stay current, so entering forces no re-round of the arena.  Inside, optimizer steps, update(),
		copy_to() and step-graph replays raise ConvasrHipError."""
		self._refuse_inside('average_parameters')
		if Fn.capturing():
			raise _lib.ConvasrHipError('WeightEMA.average_parameters: not inside a step-graph capture')
		flat = self.flat
		self._mirror()
		d16 = flat.data16
		was = [k for k, v in flat.mirror_vouchers.items() if v == W.param_version(flat._by_id[k])]
		self._exchange(d16, was)
		flat.averaged = self
		try:
			yield self
		finally:
			flat.averaged = None
			self._exchange(d16, was)

	def copy_to(self):
		"""Write the average into the parameters for good (and its mirror into the arena's): the route to model.fuse_conv_bn_eval() and to export."""
		self._refuse_inside('copy_to')
		a16, nbytes = self._mirror(), 4 * self.flat.numel

		def run(p16):
			_lib.call('convasr_copy', _lib.ptr(self.average), _lib.ptr(self.flat.data), nbytes, _lib.stream_ptr())
			if p16 is not None:
				_lib.call('convasr_copy', _lib.ptr(a16), _lib.ptr(p16), nbytes // 2, _lib.stream_ptr())
		self.flat.mirror_carried_over(run)

	def state_dict(self):
		"""decay, the update count, and the average as one tensor per parameter in the reference's shapes (flat.export_state: independent of the
		arena's element order), in flat.params order."""
		held = self.flat.data if self.flat.averaged is self else self.average  # (inside the context the two have changed places)
		return dict(format = 1, decay = self.decay, updates = self.updates, average = self.flat.export_state(held))

	def load_state_dict(self, sd):
		self._refuse_inside('load_state_dict')
		self.flat.import_state(self.average, sd['average'], 'WeightEMA.load_state_dict(average)')
		self.decay = float(sd['decay'])
		self.count[self._cur, 0] = float(sd['updates'])
		if self.average16 is not None:
			self.average16.copy_(self.average)


class _NonFinite:
	"""`not isfinite(t[i])`, evaluated (with the stream joins and the host read it takes) only when somebody asks: bool(flag)."""

	def __init__(self, t, i, engine = None):
		self.t, self.i, self.engine = t, i, engine

	def __bool__(self):
		if self.engine is not None:
			self.engine.join_comm_stream()
		return not bool(torch.isfinite(self.t[self.i]))


def train_step(model, optimizer, x, xlen, y, ylen, max_norm = 100.0, accumulate_iterations = 1, iteration = 0, world_size = 1, sync_metrics = True, device_gate = True, teacher = None, distill_weight = 0.0, distill_temperature = 1.0, distill_head = 0, ema = None):
	"""One iteration of the reference loop, train.py:745-783.

	Returns dict(loss, loss_cur, entropy, grad_norm, skipped) of 0-d device tensors (read them lazily: no forced host sync).
	The reference's inf/NaN gate (train.py:769: skip backward and the optimizer step) is applied on the device when
	device_gate is set and there is no gradient accumulation: backward still runs, but the fused optimizer kernel reads the
	(all-reduced) loss and leaves parameters and momentum untouched when it is not finite -- the same parameters as the
	reference after the iteration, without draining the GPU in the middle of every step.  With accumulation (or
	device_gate = False) the gate is the reference's host-side check.

	teacher (a models.sparse_topk dict of a teacher's logits on this batch, or a (values, indices) pair: distill.teacher_from_model,
	distill.TeacherStore.batch): the step minimises the CTC loss as above + distill_weight * mean_b(kd[b]) / accumulate_iterations, with
	kd = functional.distill_loss(logits[distill_head], teacher, olen[distill_head], distill_temperature); one backward over both loss
	vectors.  The result gains `distill`, the mean of kd (0-d, on the device), and both gates read non-finite when either mean is.
	Without a teacher the step launches exactly what it launched before the argument existed.

	ema (a WeightEMA of optimizer.flat): ema.update follows every optimizer step, with the step's device-side gate, so the average skips
	the steps the optimizer skips.  Without one the step launches exactly what it launched before the argument existed."""
	Fn.begin_step(x.device)  # the device-resident dropout key of this step (one single-thread launch; the same whether the step is launched eagerly or replayed from a graph)
	out = model(x, xlen, y = y, ylen = ylen)
	log_probs, olen, loss_vec = out['log_probs'], out['olen'], out['loss']
	# train.py:754-756 in one launch (ops.loss_head): loss = mean(loss_vec * ylen[:, 0]) / accum, loss_cur = mean(loss_vec), the mean
	# entropy, the inf/NaN flag, and d loss / d loss_vec (the vector backward() is seeded with)
	ent = M.entropy(log_probs[0].detach(), olen[0], dim = 1)
	scaler = getattr(getattr(optimizer, 'flat', None), 'loss_scaler', None)  # fp16: backward is seeded with the scaled loss's gradient (train.py:770-772)
	engine = model if hasattr(model, 'finish_gradient_sync') else None
	group = engine.group if engine is not None else None
	# The two scalar all-reduces of train.py:759-760 as one 2-element all-reduce.  With a data-parallel engine that runs
	# collectives it is NOT optional: the skip gate below must be the same number on every rank (the gradients are already
	# averaged; a rank-local inf/NaN would make one replica skip the update the others apply).
	reduce_metrics = (engine is not None and engine.collectives) or (sync_metrics and torch.distributed.is_available() and torch.distributed.is_initialized() and (world_size > 1 or sync_metrics is True))
	ranks = torch.distributed.get_world_size(group) if reduce_metrics else 1
	scalars, grad_loss_vec, skipped = ops.loss_head(loss_vec, ylen[:, 0], ent, accumulate_iterations, loss_scaler = None if scaler is None else scaler.current, metric_scale = 1.0 / ranks)
	skipped = skipped[0]
	if reduce_metrics:
		# SUM of (local mean / world) = the mean over ranks, with no divide kernel behind it.  With an engine the collective runs on the
		# engine's communication stream like the gradient buckets (the fused optimizer step, which reads the reduced loss as its skip
		# gate, is ordered behind that stream by finish_gradient_sync); the host-visible flag is evaluated only if somebody looks.
		if engine is not None and engine.collectives:
			engine.all_reduce_async(scalars[1:3])
		else:
			torch.distributed.all_reduce(scalars[1:3], op = torch.distributed.ReduceOp.SUM, group = group)
		skipped = _NonFinite(scalars, 1, engine)
	loss_cur = scalars[1]
	res = dict(loss = scalars[0], loss_cur = loss_cur, entropy = scalars[2], grad_norm = None, skipped = skipped)
	if 'star_frames' in out:  # model.ctc_star is set: per head, the expected frames every gap's star absorbed (B, S_max + 1)
		res['star_frames'] = out['star_frames']
	for name in ('mwer_loss', 'mwer_expected_risk', 'mwer_best_risk', 'mwer_skipped'):  # model.ctc_mwer is set: the term and its statistics per utterance, and the skipped utterances
		if name in out:
			res[name] = out[name].detach()
	gate_source = scalars
	losses, seeds = [loss_vec], [grad_loss_vec]
	if teacher is not None:
		kd = Fn.distill_loss(out['logits'][distill_head], teacher, olen[distill_head], distill_temperature)
		distill = kd.detach().mean()
		if reduce_metrics:
			distill = distill / ranks
			torch.distributed.all_reduce(distill, op = torch.distributed.ReduceOp.SUM, group = group)
			if engine is not None:
				engine.join_comm_stream()  # the CTC means' all-reduce runs on the engine's stream: the gate below reads its result
		res['distill'] = distill
		# one number that is non-finite when either mean is: what the fused optimizer step and the host-side check read (0 * inf = NaN)
		gate_source = torch.stack([scalars[0], scalars[1] + distill * 0.0])
		res['skipped'] = skipped = _NonFinite(gate_source, 1, engine) if reduce_metrics else skipped | ~torch.isfinite(distill)
		if distill_weight != 0.0:
			seed = float(distill_weight) / (kd.shape[0] * accumulate_iterations)
			kd_seed = torch.full_like(kd, seed) if scaler is None else scaler.current[0] * seed * torch.ones_like(kd)
			losses.append(kd)
			seeds.append(kd_seed)
	gate = None
	if device_gate and accumulate_iterations == 1 and hasattr(optimizer, 'flat'):
		gate = gate_source[1:2]
	elif bool(skipped):
		res['skipped'] = True
		return res
	last_of_group = iteration % accumulate_iterations == 0
	backward = (lambda: loss_vec.backward(grad_loss_vec)) if len(losses) == 1 else (lambda: torch.autograd.backward(losses, seeds))
	if engine is not None and not last_of_group:
		with engine.no_sync():
			backward()
	else:
		backward()
	Fn.join_side_streams()  # weight gradients computed on the side stream are final from here on
	if last_of_group:
		if engine is not None:
			engine.finish_gradient_sync()
		flat = optimizer.flat
		own_norm = getattr(optimizer, 'clips_in_step', False)  # (NovoGrad forms the gradient norm inside its fused step: no separate reduction pass over the arena)
		if own_norm:
			flat.finalize_grads()
			flat.clip = (None, float(max_norm))
		else:
			res['grad_norm'] = flat.clip_grad_norm_(max_norm)
		if gate is not None:
			optimizer.step(loss_gate = gate)
		else:
			optimizer.step()
		if ema is not None:
			ema.update(loss_gate = gate)
		if own_norm:
			res['grad_norm'] = optimizer.total_norm[0]
		optimizer.zero_grad()
	return res


_HIP_NODE_TYPES = {0: 'kernel', 1: 'memcpy', 2: 'memset', 3: 'host', 4: 'graph', 5: 'empty', 6: 'wait_event', 7: 'event_record', 8: 'ext_sem_signal', 9: 'ext_sem_wait', 10: 'mem_alloc', 11: 'mem_free', 12: 'memcpy_from_symbol', 13: 'memcpy_to_symbol'}  # hipGraphNodeType
_hip_runtime = []


def capture_node_kinds(device):
	"""{node type: count} of the graph being captured on the current stream of `device` (hipStreamGetCaptureInfo_v2 -> hipGraphGetNodes ->
	hipGraphNodeGetType, over the HIP runtime torch has loaded), or None when the stream is not capturing / the runtime cannot be asked."""
	import ctypes
	try:
		if not _hip_runtime:
			_hip_runtime.append(ctypes.CDLL('libamdhip64.so'))
		hip = _hip_runtime[0]
		status, gid, graph, deps, ndeps = ctypes.c_int(0), ctypes.c_ulonglong(0), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(0)
		stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
		if hip.hipStreamGetCaptureInfo_v2(stream, ctypes.byref(status), ctypes.byref(gid), ctypes.byref(graph), ctypes.byref(deps), ctypes.byref(ndeps)) != 0 or status.value != 1 or not graph:
			return None
		n = ctypes.c_size_t(0)
		if hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) != 0:
			return None
		nodes = (ctypes.c_void_p * max(n.value, 1))()
		if hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) != 0:
			return None
		kinds = {}
		for i in range(n.value):
			t = ctypes.c_int(-1)
			hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t))
			name = _HIP_NODE_TYPES.get(t.value, str(t.value))
			kinds[name] = kinds.get(name, 0) + 1
		return kinds
	except (OSError, AttributeError):
		return None


class GraphedTrainStep:
	"""train_step(model, optimizer, x, xlen, y, ylen) with accumulate_iterations = 1, replayed from a HIP graph: one graph per batch shape
	(x.shape, y.shape -- a bucketed loader that pads every batch of a bucket to the bucket's ceiling, datasets.bucket_ceiling, produces
	about a dozen), captured after `warmup` eager steps of that shape.  A JasperNetLarge step is ~530 kernel launches and ~19 ms of
	Python for ~40 ms of GPU work; a replay is one call.

	What makes the captured step a faithful replay (tests/test_full_size_and_step_graphs_gpu.py compares 20 / 24 steps bit for bit with the eager path):
	* everything that changes from step to step is read from device memory when the kernels RUN -- the dropout step key
	  (functional.begin_step), the loss scaler, the optimizer's step counters / EMAs, the learning rate (`optimizer.lr_dev`, refreshed here
	  whenever the host's scheduler changed param_groups[0]['lr']), the device-side skip gates;
	* double-buffered device state is handed back to the buffer the graph reads (LossScaler.advance, optimizers._advance);
	* every buffer a captured kernel touches is either persistent (parameters, arenas, optimizer state, packed weights) or was allocated
	  inside the capture, from a memory pool all graphs of this object share (they never run concurrently): functional.CAPTURING turns the
	  per-module / per-stream caches off;
	* the capture is one chain of nodes (linear = True: side streams off while capturing; linear = False forks and joins the weight-gradient
	  side stream and the dgrad-weight prepack stream inside the capture -- slower on ROCm 7.2, see _capture).

	Inputs are copied into the graph's static buffers (one device-to-device copy each; pass the static buffers themselves -- .inputs(key)
	-- to skip it).  Returned metrics are the graph's static output tensors: read them before the next call with the same shape.
	A data-parallel engine is captured WITH its collectives when they are RCCL's (parallel.DataParallelEngine.capturable): the bucket
	all-reduces are recorded on the communication stream, which forks off the capturing stream at the buckets' ready events and rejoins it in
	finish_gradient_sync, so a replayed step overlaps the exchange with the backward pass like the eager one and costs the host one launch
	(eagerly every rank spends ~4 / ~19 ms of Python per Wav2Letter / JasperNetLarge step).  gloo engines (host waits) stay eager: the call
	falls through to train_step (with this object's world_size / sync_metrics).

	ema (a WeightEMA of optimizer.flat): every step, eager or replayed, is followed by ema.update with the step's gate; the captured step holds
	it as kernel nodes (the update, then the hand-back of its counter to the row the graph reads), nothing else."""

	def __init__(self, model, optimizer, max_norm = 100.0, warmup = 1, enabled = True, linear = os.environ.get('CONVASR_GRAPH_FORKED') != '1', max_graphs = 64, world_size = 1, sync_metrics = True, ema = None):
		self.model, self.optimizer, self.max_norm, self.warmup, self.linear = model, optimizer, max_norm, max(int(warmup), 1), linear
		self.ema = ema  # a WeightEMA of optimizer.flat, or None: its update is captured behind the optimizer step (kernel nodes: the update and the hand-back of its counter)
		self._refuse_mwer()
		self.world_size, self.sync_metrics = world_size, sync_metrics  # (for the eager fall-through of a data-parallel engine: what train_step averages the logged metrics over)
		self.max_graphs = max_graphs  # batch shapes beyond this many stay eager (a loader that does not pad to bucket ceilings produces a new shape per batch: every capture keeps its static inputs and outputs alive)
		engine = model if hasattr(model, 'finish_gradient_sync') else None
		self.enabled = bool(enabled) and (engine is None or engine.capturable)  # (an engine whose collectives are RCCL's is captured with them: the communication stream forks off and rejoins inside the graph; gloo waits on the host and stays eager)
		if self.enabled and engine is not None and engine.collectives:
			engine.enable_capture()  # (a rendezvous of all ranks: the engine's own RCCL communicator, through which the captured collectives go -- parallel.DataParallelEngine.enable_capture)
		self.graphs, self.seen = {}, {}
		self.pool = None
		self.epoch = W.structure_epoch()
		self.replays = self.captures = self.eager_steps = 0
		self.non_kernel_nodes = os.environ.get('CONVASR_GRAPH_FENCE') == '1'  # does any captured step hold a memset / memcpy / ... node (see _fence_transition)?
		self._lr = None

	@staticmethod
	def key_of(x, xlen, y, ylen):
		return (tuple(x.shape), x.dtype, tuple(xlen.shape), tuple(y.shape), y.dtype, tuple(ylen.shape))

	def inputs(self, key):
		g = self.graphs.get(key)
		return None if g is None else g['static']

	def _fence_transition(self, device, eager):
		"""A host wait for the stream wherever an eagerly launched step meets a replayed one (either order) -- armed only when a captured step
		contains a node that is not a kernel.  Round 6 (profiles/r06_interleave_race.txt): with the order A A B A B B C A B C A on a small Wav2Letter
		(AdamW, bf16, max_graphs = 2: C stays eager) the replay of A after the second eager C computed a different loss in most runs.  Root cause:
		the MEMSET node the capture recorded for convasr_signal_absmax's hipMemsetAsync (the first node of the step).  On ROCm 7.2 it is not
		reliably ordered against the graph's own next kernel (the atomicMax reduction into the words it clears) when the replay follows eagerly
		launched work; the utterances' maxima then come out cleared and normalize_signal scales by 1 / eps.  With that clear (and convasr_copy,
		a hipMemcpyAsync before) turned into kernels every captured step consists of kernel nodes only (tests/test_full_size_and_step_graphs_gpu.py
		counts them) and the sequence is bit-identical to the eager run with no fence (6 of 6; 2 of 6 with the memset node back in).  The fence stays
		as the guard for graphs that do contain memset / memcpy nodes (a user module's torch ops may record them): one host wait per transition,
		nothing on the replay-to-replay path."""
		if self.graphs and self.non_kernel_nodes and getattr(self, '_last_eager', None) is not None and self._last_eager != eager and device.type == 'cuda':
			torch.cuda.current_stream(device).synchronize()
		self._last_eager = eager

	def _eager(self, x, xlen, y, ylen, iteration):
		self.eager_steps += 1
		self._fence_transition(x.device, eager = True)
		return train_step(self.model, self.optimizer, x, xlen, y, ylen, max_norm = self.max_norm, iteration = iteration, world_size = self.world_size, sync_metrics = self.sync_metrics, ema = self.ema)

	def _sync_lr(self):
		lr = float(self.optimizer.param_groups[0]['lr'])
		if self.optimizer.lr_dev is None:
			self.optimizer.lr_dev = torch.empty(1, dtype = torch.float32, device = self.optimizer.flat.data.device)
			self._lr = None
		if lr != self._lr:
			self.optimizer.lr_dev.fill_(lr)  # (outside the graph, only when the scheduler moved: one tiny launch)
			self._lr = lr

	def _capture(self, key, x, xlen, y, ylen, iteration):
		dev = x.device
		static = tuple(t.clone() for t in (x, xlen, y, ylen))
		if self.pool is None:
			self.pool = torch.cuda.graph_pool_handle()
		graph = torch.cuda.CUDAGraph()
		opt = self.optimizer
		steps0 = opt.steps
		self._sync_lr()
		net = M.master_module(self.model)
		cached = getattr(net, '_dgrad_weights', None)
		if cached is not None and cached[0] == W.structure_epoch():
			W.prewarm_dgrad_pack(cached[1], net.compute_dtype)  # (a host-to-device table copy: not possible inside the capture)
		# double-buffered device state (NovoGrad's EMAs, AdamW's applied-step counter, the loss scaler): the rows stop swapping for good --
		# this graph, and every later eager step, hands the new state back to the row that is current now
		opt._pinned = True
		W.GRAPHS_CAPTURED[0] = True
		if getattr(opt.flat, 'loss_scaler', None) is not None:
			opt.flat.loss_scaler.pinned = True
		if self.ema is not None:
			self.ema.pin()
		# every version-keyed packed copy (padded-Cout forward operands, the folded prologue, the padded head, fp32 / split operands) is
		# declared stale, so that ALL per-step pack launches are recorded in the graph: a copy that happens to be current now -- a validation
		# forward ran since the last optimizer step -- would otherwise get no pack node and go stale under replays
		W.force_repack()
		torch.cuda.synchronize(dev)
		# The captured step is ONE chain of nodes unless linear = False: the weight-gradient side stream and the dgrad-weight prepack stream are
		# switched off for the capture.  Measured on ROCm 7.2 (profiles/r05_graph_ab.json): a graph with forked branches replays 2 % SLOWER
		# than the same nodes in one chain (the runtime spreads the branches over several queues and pays for the cross-queue signals; with
		# DEBUG_HIP_FORCE_GRAPH_QUEUES=1 the forked capture matches the linear one), and never reaches the eager side stream's overlap.
		side, prepack = dict(Fn._side_streams), W.PREPACK
		if self.linear:
			Fn.join_side_streams()
			for k in Fn._side_streams:
				Fn._side_streams[k] = None
			W.PREPACK = False
		Fn.CAPTURING[0] = True
		try:
			with torch.cuda.graph(graph, pool = self.pool):
				res = train_step(self.model, opt, *static, max_norm = self.max_norm, iteration = iteration, world_size = self.world_size, sync_metrics = self.sync_metrics, ema = self.ema)
				kinds = capture_node_kinds(dev)
		finally:
			Fn.CAPTURING[0] = False
			Fn._side_streams.update(side)
			W.PREPACK = prepack
		opt.steps = steps0  # (nothing ran: the replay below is this step)
		self.graphs[key] = dict(graph = graph, static = static, res = res, node_kinds = kinds)
		if kinds is None or any(k != 'kernel' for k in kinds):
			self.non_kernel_nodes = True  # (arms _fence_transition; a capture that cannot be inspected is treated like one that holds other nodes)
		self.captures += 1

	def _refuse_mwer(self):
		if getattr(M.master_module(self.model), 'ctc_mwer', None) is not None:
			raise ValueError('GraphedTrainStep: the model has ctc_mwer set; its N-best beam search allocates per call and reads a length on the host, so the MWER route is eager only: use train_step')

	def __call__(self, x, xlen, y, ylen, iteration = 0):
		self._refuse_mwer()
		if not self.enabled:
			return self._eager(x, xlen, y, ylen, iteration)
		if self.epoch != W.structure_epoch():  # conv modules were replaced (fuse_conv_bn_eval): the captured pointers are stale
			self.graphs, self.seen, self.epoch = {}, {}, W.structure_epoch()
		key = self.key_of(x, xlen, y, ylen)
		g = self.graphs.get(key)
		if g is None:
			n = self.seen.get(key, 0)
			if n < self.warmup or self.optimizer.steps == 0 or len(self.graphs) >= self.max_graphs:
				self.seen[key] = n + 1
				return self._eager(x, xlen, y, ylen, iteration)
			self._capture(key, x, xlen, y, ylen, iteration)
			g = self.graphs[key]
		for dst, src in zip(g['static'], (x, xlen, y, ylen)):
			if dst.data_ptr() != src.data_ptr():
				_lib.call('convasr_copy', _lib.ptr(src if src.is_contiguous() else src.contiguous()), _lib.ptr(dst), dst.numel() * dst.element_size(), _lib.stream_ptr())
		self._sync_lr()
		opt = self.optimizer
		W.join_prepack(x.device)  # (side streams an eager step may have left running are joined before the graph is launched)
		self._fence_transition(x.device, eager = False)
		Fn.join_side_streams()
		opt.flat.mirror_carried_over(lambda p16: g['graph'].replay())  # (the same version bookkeeping an eager optimizer launch gets: the 16-bit mirror stays current, other packed copies go stale)
		opt.steps += 1
		self.replays += 1
		return g['res']


def train_epoch(model, optimizer, batches, sampler = None, scheduler = None, iteration = 0, world_size = 1, max_norm = 100.0, accumulate_iterations = 1, max_iterations = None, on_step = None, graphs = None, teacher_fn = None, distill_weight = 0.0, distill_temperature = 1.0, distill_head = 0, ema = None):
	"""The body of the reference's epoch loop (train.py:739-808) over an iterable of (meta, s, x, xlen, y, ylen) batches whose
	tensors are already on the device (convasr_amd.datasets.gpu_batches): train_step, scheduler.step(iteration) after every
	optimizer step (train.py:783), iteration += 1, sampler.batch_idx += world_size (train.py:807-808, what makes a resumed
	epoch start where it stopped).  Metrics stay on the device; on_step(iteration, batch, result) may read them.
	teacher_fn(batch) -> the teacher of train_step for the batch (meta, s, x, xlen, y, ylen), with distill_weight / distill_temperature /
	distill_head handed on; not together with graphs (GraphedTrainStep does not distil): ValueError.
	ema: a WeightEMA handed on to train_step; a GraphedTrainStep carries its own (GraphedTrainStep(..., ema = ema)), and the two must agree: ValueError.
	Returns the next iteration number."""
	if graphs is not None and teacher_fn is not None:
		raise ValueError('train_epoch: graphs and teacher_fn do not combine (GraphedTrainStep does not capture the distillation term)')
	if graphs is not None and ema is not None and graphs.ema is not ema:
		raise ValueError('train_epoch: the step graphs were built without this WeightEMA: pass it as GraphedTrainStep(..., ema = ema)')
	for meta, s, x, xlen, y, ylen in batches:
		if graphs is not None and accumulate_iterations == 1 and world_size == 1:
			res = graphs(x, xlen, y, ylen, iteration = iteration)  # a GraphedTrainStep(model, optimizer, max_norm): replayed per batch shape
		elif teacher_fn is not None:
			res = train_step(model, optimizer, x, xlen, y, ylen, max_norm = max_norm, accumulate_iterations = accumulate_iterations, iteration = iteration, world_size = world_size, sync_metrics = world_size > 1,
				teacher = teacher_fn((meta, s, x, xlen, y, ylen)), distill_weight = distill_weight, distill_temperature = distill_temperature, distill_head = distill_head, ema = ema)
		else:
			res = train_step(model, optimizer, x, xlen, y, ylen, max_norm = max_norm, accumulate_iterations = accumulate_iterations, iteration = iteration, world_size = world_size, sync_metrics = world_size > 1, ema = ema)
		# train.py:769-783: the scheduler steps only inside the not-skipped branch.  Where the host knows the verdict (a host-side gate
		# returned skipped = True) the reference's behaviour is reproduced exactly; with the device-side gate the host does not wait
		# for it, and after a skipped iteration the next step's lr is one scheduler tick ahead of the reference's
		if scheduler is not None and iteration % accumulate_iterations == 0 and res['skipped'] is not True:
			scheduler.step(iteration)
		if on_step is not None:
			on_step(iteration, (meta, s, x, xlen, y, ylen), res)
		iteration += 1
		if sampler is not None:
			sampler.batch_idx += world_size
		if max_iterations is not None and iteration >= max_iterations:
			break
	return iteration


def _finite_mean(values):
	"""metrics.nanmean (metrics.py:247-253) over one CPU tensor: the mean of the finite values, summed in order as Python floats, -1.0 when
	there are none."""
	vals = [v for v in values.tolist() if math.isfinite(v)]
	return sum(vals) / len(vals) if vals else -1.0


def evaluate_model(model, batches, tokenizer, decoder = None, blank_amount_to_space = 10, return_text = False, error_analyzer = None, logits_topk = None, logits_dtype = torch.float16, ema = None):
	"""One validation set through the reference's apply_model + evaluate_model (train.py:119-300), for the first target head.

	batches yields (meta, s, x, xlen, y, ylen) with the tensors on the device, as for train_epoch.  Per batch, under no_grad with the model
	in evaluation mode: the forward with y / ylen (the per-utterance CTC loss), models.entropy and models.weighted_mean_entropy of
	log_probs[0] / olen[0], the hypotheses -- ops.argmax + ops.ctc_greedy_collapse (GreedyCTCGenerator's rules, blank_amount_to_space) when
	decoder is None, else the topk hypotheses of a decoders.BeamSearchDecoder -- and their CER / WER against y[:, 0] / ylen[:, 0] through
	metrics.token_cer_wer (tokenizer: CharTokenizerLegacy or another one-character lowercase tokenizer; tokenizer.eps_id / space_id).  With
	topk > 1 also cer_oracle / wer_oracle, the minimum over the hypotheses the search filled.

	The score is against the ENCODED targets y, which is what the model is trained on; the reference scores against
	pipeline.preprocess(meta['ref']).  The two differ only where the tokenizer maps a character to '*' (unk).  For the reference's string
	semantics, decode and use metrics.cer_wer.

	Returns dict(loss, entropy, cer, wer[, cer_oracle, wer_oracle]) of aggregates -- the mean over the finite per-utterance values, -1.0
	when there are none (metrics.nanmean) -- and `utterances`: per-utterance CPU tensors in batch order (loss, entropy, uncertainty, cer,
	wer[, cer_oracle, wer_oracle]); with return_text also `hyp`, the best hypothesis of every utterance as transcribe.join would give it.
	Everything reaches the host in one copy at the end.  The hypotheses are scored as (B, K, T) token rows, T the batch's output frames, so a
	batch of more than 16,383 output frames (ops.edit_distance's envelope) takes metrics.token_cer_wer's long route: ops.edit_distance_long, up to 131,071 frames,
	with one extra round trip of the tokens for the word ids.  model.training is restored on return; parameters, batch-norm statistics, torch's
	RNG and the dropout generator's offsets are left as they were.

	error_analyzer: a metrics.ErrorAnalyzer, or None.  With one, the best hypothesis and the decoded target y[:, 0] of every utterance (their
	tokens ride in the same single copy) go through error_analyzer.analyze_batch(detailed = True) -- the reference's validation analysis
	(train.py:239-300 there: alignment, word error tags, wordwise / filtered / pseudo / vocabness metrics per config), a constant number of
	launches for the whole set.  The result gains `analysis`, error_analyzer.aggregate of the per-utterance dicts, and
	utterances['analysis'], those dicts; with return_text also `ref`, the decoded targets.  Without one the result is what it was.

	logits_topk = k (the reference's --logits / --logits-topk): utterances['logits'] is a list of per-utterance dicts, in batch order, each
	with `values` (k, olen_b) in logits_dtype and `indices` (k, olen_b) (uint8 up to 256 classes, else int16): the k largest logits of
	every frame of the utterance's own olen_b frames (ops.topk_frames on the first head's logits; the padding is cut on the device, the
	reference's unpad) -- what distill.TeacherStore.add_utterances takes.  They reach the host in one more copy at the end.  Without it the
	result is what it was.

	ema: a WeightEMA of the model's arena, or None.  With one the whole pass runs inside ema.average_parameters(): the averaged parameters with
	the model's current batch-norm running statistics; the raw parameters are back on return, also after an exception.  Without one the pass
	launches what it launched before the argument existed."""
	from . import metrics
	training, drop_offset = model.training, Fn._DropoutState.offset
	cols, hyp_tokens, ref_tokens, n_batches = [], [], [], 0
	top_values, top_indices, top_olen = [], [], []
	model.eval()
	try:
		with torch.no_grad(), (ema.average_parameters() if ema is not None else contextlib.nullcontext()):
			for meta, s, x, xlen, y, ylen in batches:
				out = model(x, xlen, y = y, ylen = ylen)
				lp, olen = out['log_probs'][0], out['olen'][0]
				ent, unc = M.entropy(lp, olen, dim = 1), M.weighted_mean_entropy(lp, olen)
				if decoder is None:
					tokens, lengths = ops.ctc_greedy_collapse(ops.argmax(lp), olen, tokenizer.eps_id, tokenizer.space_id, blank_amount_to_space)
					tokens, lengths, filled = tokens.unsqueeze(1), lengths.unsqueeze(1), None
				else:
					tokens, _, lengths, log_prob = decoder.decode_with_scores(lp, olen)
					filled = torch.isfinite(log_prob)
				c, w = metrics.token_cer_wer(tokens, lengths, y[:, 0], ylen[:, 0], tokenizer.space_id)
				col = [out['loss'].double(), ent.double(), unc.double(), c[:, 0], w[:, 0]]
				if tokens.shape[1] > 1:
					inf = torch.full_like(c, float('inf'))
					col += [torch.where(filled, c, inf).amin(dim = 1), torch.where(filled, w, inf).amin(dim = 1)]
				cols.append(torch.stack(col))
				if return_text or error_analyzer is not None:
					hyp_tokens.append((tokens[:, 0], lengths[:, 0]))
				if error_analyzer is not None:
					ref_tokens.append((y[:, 0], ylen[:, 0].to(torch.int64)))
				if logits_topk is not None:
					lg = out['logits'][0]
					top = M.sparse_topk(lg.float(), logits_topk, dim = 1, indices_dtype = torch.uint8 if lg.shape[1] <= 256 else torch.int16, values_dtype = logits_dtype)
					keep = torch.arange(lg.shape[2], device = lg.device).unsqueeze(0) < olen.unsqueeze(1)  # (B, T): the utterance's own frames
					top_values.append(top['values'].permute(0, 2, 1)[keep])  # (sum olen, k), utterance after utterance
					top_indices.append(top['indices'].permute(0, 2, 1)[keep])
					top_olen.append(olen)
				n_batches += 1
			if not n_batches:
				raise ValueError('evaluate_model: no batches')
			table = torch.cat(cols, dim = 1)
			# one device-to-host copy: the per-utterance table (fp64 bits) and, for the text, the best hypotheses' lengths and tokens
			parts = [table.contiguous().view(torch.int64).flatten()]
			for t, l in hyp_tokens + ref_tokens:
				parts += [l, t.flatten()]
			if logits_topk is not None:
				parts.append(torch.cat(top_olen).to(torch.int64))
			host = torch.cat(parts).cpu()
			if logits_topk is not None:
				top_values, top_indices = torch.cat(top_values).cpu(), torch.cat(top_indices).cpu()
	finally:
		model.train(training)
		Fn._DropoutState.offset = drop_offset
	n_rows = table.shape[0]
	table = host[:table.numel()].view(torch.float64).view(n_rows, -1)
	names = ['loss', 'entropy', 'uncertainty', 'cer', 'wer'] + (['cer_oracle', 'wer_oracle'] if n_rows > 5 else [])
	utt = {k: table[i].clone() for i, k in enumerate(names)}
	utt['loss'], utt['entropy'], utt['uncertainty'] = utt['loss'].float(), utt['entropy'].float(), utt['uncertainty'].float()
	res = {k: _finite_mean(utt[k]) for k in names if k != 'uncertainty'}
	res['utterances'] = utt
	if logits_topk is not None:
		counts = host[-table.shape[1]:].tolist()
		utt['logits'] = [dict(values = v.t(), indices = i.t()) for v, i in zip(top_values.split(counts), top_indices.split(counts))]
	if return_text or error_analyzer is not None:
		texts, pos = [], table.numel()
		for t, l in hyp_tokens + ref_tokens:
			B, T = t.shape
			lens = host[pos:pos + B].tolist()
			toks = host[pos + B:pos + B + B * T].view(B, T).tolist()
			pos += B + B * T
			texts += [tokenizer.decode([row[:n]])[0].strip() for row, n in zip(toks, lens)]
		hyp, ref = texts[:table.shape[1]], texts[table.shape[1]:]
		if return_text:
			res['hyp'] = hyp
		if error_analyzer is not None:
			analysis = error_analyzer.analyze_batch(hyp, ref, detailed = True)
			res['analysis'] = error_analyzer.aggregate(analysis)
			utt['analysis'] = analysis
			if return_text:
				res['ref'] = ref
	return res
