"""float64 restatement of the fused optimizer tail: sumsq, sgd_step, adamw_step (convasr_amd/csrc/misc.hip), novograd_step (csrc/next.hip) and
the loss-scaler helpers loss_scale_read / loss_scale_advance (csrc/common.h), plain torch / numpy on the CPU.  Nothing here loads the library.

The functions mirror the launchers' arguments (convasr_amd.ops) but return what a launch writes instead of writing it.  Arrays are the fp32
values the device holds, up-converted; hyper-parameters are the fp32 values the C ABI receives (a `float` argument), up-converted; all
ELEMENTWISE arithmetic is float64.

What the kernels DECIDE per launch in fp32 is restated in exactly that precision and order (numpy float32 scalars), because a decision has
one right answer, bit for bit, and a float64 "improvement" of it would be another operation:
  inv       = 1.f / scaler[LS_SCALE]                       (no scaler: 1)
  gs        = grad_scale * inv
  total     = (float)sqrt(sumsq) * gs                      (sqrt in double, one rounding to fp32, one fp32 product)
  c         = max_norm / (total + 1e-6f)
  clip      = (c < 1 ? c : 1) * gs                         (only when max_norm > 0 and there is a sumsq; else clip = gs.  A NaN c compares
                                                            false: 1)
  gated     = loss_gate given and not |loss_gate| < inf
  overflow  = scaler given, window > 0, and not |sumsq| < inf
  the loss scaler's eight floats (loss_scale_advance)
  the applied-step counters: AdamW's t0 + 1.f (which stays at 2^24 by fp32 rounding), NovoGrad's min(applied + 1.f, 2^24)
  NovoGrad's `first`: the argument, or (first < 0) applied == 0 read from behind the EMAs
Everything else -- bias corrections, EMAs, denominators, the updates -- is float64.

A gated or overflowed step changes nothing except what the kernels document: NovoGrad's EMAs (and counter) are carried into ema_out,
AdamW's step_out = step_in, the scaler state advances (gated: it is copied).  The functions return the inputs' own values then
(`applied` False), so a caller can compare bit for bit.
tests/test_optim_ref.py holds all of this to torch.optim in float64, the oracle, the committed golden and apex's update_scale()."""
import numpy as np
import torch

LS_SCALE, LS_UNSKIPPED, LS_OVERFLOW, LS_WINDOW, LS_MIN, LS_MAX, LS_FACTOR, LS_SKIPPED_STEPS = range(8)  # csrc/common.h
LOSS_SCALER_FLOATS = 8
COUNTER_CAP = 16777216.0  # 2^24: the last fp32 whose successor is still an integer

f32 = np.float32


def f64(t):
	return None if t is None else t.detach().to(device = 'cpu', dtype = torch.float64)


def r32(v):
	"""the value a `float` argument of the C ABI holds, as a Python float"""
	return float(f32(v))


def scalar(t):
	"""a 1-element device / host tensor (sumsq, loss gate, lr_dev, counter) or a number -> Python float, exactly"""
	return None if t is None else float(t.detach().cpu().double().reshape(-1)[0]) if isinstance(t, torch.Tensor) else float(t)


def state32(scaler):
	return None if scaler is None else scaler.detach().cpu().to(torch.float32).numpy().copy()


# ------------------------------------------------------------------------------------------------ loss scaler (csrc/common.h), exact

def scaler_state(scale, window, factor = 2.0, min_scale = 0.0, max_scale = 2.0 ** 24, unskipped = 0.0, skipped_steps = 0.0):
	"""the eight floats convasr_amd.train.LossScaler keeps (window 0: static scale)"""
	return torch.tensor([scale, unskipped, 0.0, window, min_scale, max_scale, factor, skipped_steps], dtype = torch.float32)


def loss_scale_overflow(scaler, norm_sq):
	"""loss_scale_read's verdict: a dynamic scaler (window > 0) and a squared gradient norm that is inf or NaN"""
	if scaler is None:
		return False
	s = state32(scaler)
	return bool(s[LS_WINDOW] > 0) and not (abs(norm_sq) < float('inf'))


def loss_scale_inv(scaler):
	"""1.f / scale in fp32 (1 without a scaler)"""
	with np.errstate(all = 'ignore'):
		return f32(1) if scaler is None else f32(1) / state32(scaler)[LS_SCALE]


def loss_scale_advance(scaler, overflow, gated):
	"""the state after one optimizer launch, fp32 bit for bit.  gated (non-finite LOSS): a copy.  Otherwise the overflow flag is set; a
	static scaler (window <= 0) stops there; a dynamic one follows apex's update_scale(): overflow -> scale = max(min, scale / factor),
	unskipped = 0, ++skipped_steps; else ++unskipped; then unskipped >= window -> scale = min(max, scale * factor), unskipped = 0."""
	s = state32(scaler)
	out = s.copy()
	if gated:
		return torch.from_numpy(out)
	out[LS_OVERFLOW] = f32(1 if overflow else 0)
	if not s[LS_WINDOW] > 0:
		return torch.from_numpy(out)
	scale, unskipped = s[LS_SCALE], s[LS_UNSKIPPED]
	with np.errstate(all = 'ignore'):
		if overflow:
			scale, unskipped = np.maximum(s[LS_MIN], scale / s[LS_FACTOR]), f32(0)
			out[LS_SKIPPED_STEPS] = s[LS_SKIPPED_STEPS] + f32(1)
		else:
			unskipped = unskipped + f32(1)
		if unskipped >= s[LS_WINDOW]:
			scale, unskipped = np.minimum(s[LS_MAX], scale * s[LS_FACTOR]), f32(0)
	out[LS_SCALE], out[LS_UNSKIPPED] = scale, unskipped
	return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------ launch-wide decisions, exact

def is_gated(loss_gate):
	return loss_gate is not None and not (abs(scalar(loss_gate)) < float('inf'))


def clip_coef(sumsq, max_norm, grad_scale = 1.0, scaler = None):
	"""the factor every gradient element is multiplied by, as an fp32 value (Python float): clip_grad_norm_'s coefficient x the pending
	gradient scale x 1 / loss scale, in the kernels' fp32 order (module docstring)"""
	with np.errstate(all = 'ignore'):
		gs = f32(grad_scale) * loss_scale_inv(scaler)
		clip = f32(1)
		if sumsq is not None and max_norm is not None and f32(max_norm) > 0:
			total = f32(np.sqrt(np.float64(scalar(sumsq)))) * gs
			c = f32(max_norm) / (total + f32(1e-6))
			clip = c if c < 1 else f32(1)
		return float(clip * gs)


def counter_next(applied):
	"""fp32 applied + 1, capped at 2^24 (AdamW's plain t0 + 1.f gives the same values: 2^24 + 1 rounds back to 2^24)"""
	return float(min(f32(applied) + f32(1), f32(COUNTER_CAP)))


# ------------------------------------------------------------------------------------------------ gradient norm

def sumsq(g):
	"""sum of squares, float64 (0-d)"""
	return f64(g).pow(2).sum()


def grad_norm(sumsq_value, norm_scale = 1.0, scaler = None):
	"""norm_out of the sumsq launch / total_norm of novograd_step: sqrt(sum of squares) x scale / loss scale, float64"""
	inv = 1.0 if scaler is None else 1.0 / float(state32(scaler)[LS_SCALE])
	return float(np.sqrt(np.float64(scalar(sumsq_value)))) * r32(norm_scale) * inv


# ------------------------------------------------------------------------------------------------ SGD (torch.optim.SGD + clip_grad_norm_)

def sgd_step(p, g, buf, sumsq, max_norm, lr, momentum, weight_decay, nesterov, first, loss_gate = None, grad_scale = 1.0, scaler = None, lr_dev = None):
	"""-> dict(p, buf, grad_out, scaler_out, applied).  gc = g clip; d = gc + wd p; momentum != 0: buf = first ? d : mom buf + d,
	d = nesterov ? d + mom buf : buf; p -= lr d.  grad_out = gc.  momentum == 0: buf is returned as given (the kernel never touches it).
	sumsq: the fp64 sum of squares the launch is handed (None: no clipping, and no scaler)."""
	pd, gd, bd = f64(p), f64(g), f64(buf)
	lr = scalar(lr_dev) if lr_dev is not None else r32(lr)
	mom, wd = r32(momentum), r32(weight_decay)
	gated = is_gated(loss_gate)
	overflow = loss_scale_overflow(scaler, scalar(sumsq) if sumsq is not None else 0.0)
	out = dict(p = pd, buf = bd, grad_out = None, scaler_out = None if scaler is None else loss_scale_advance(scaler, overflow, gated), applied = not (gated or overflow))
	if not out['applied']:
		return out
	gc = gd * clip_coef(sumsq, max_norm, grad_scale, scaler)
	d = gc + wd * pd
	if mom != 0:
		bd = d if first else mom * bd + d
		d = d + mom * bd if nesterov else bd
	out.update(p = pd - lr * d, buf = bd, grad_out = gc)
	return out


# ------------------------------------------------------------------------------------------------ AdamW (torch.optim.AdamW + clip_grad_norm_)

def adamw_step(p, g, exp_avg, exp_avg_sq, sumsq, max_norm, lr, beta1, beta2, eps, weight_decay, step_in, loss_gate = None, grad_scale = 1.0, scaler = None, lr_dev = None):
	"""-> dict(p, exp_avg, exp_avg_sq, step_out, scaler_out, applied).  t = step_in + 1; p *= 1 - lr wd; m = b1 m + (1 - b1) gc;
	v = b2 v + (1 - b2) gc^2; p -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps).  step_in: the count of steps APPLIED so far (fp32);
	a skipped launch hands it on unchanged."""
	pd, gd, m, v = f64(p), f64(g), f64(exp_avg), f64(exp_avg_sq)
	lr = scalar(lr_dev) if lr_dev is not None else r32(lr)
	b1, b2, eps, wd = r32(beta1), r32(beta2), r32(eps), r32(weight_decay)
	t0 = scalar(step_in)
	gated = is_gated(loss_gate)
	overflow = loss_scale_overflow(scaler, scalar(sumsq) if sumsq is not None else 0.0)
	out = dict(p = pd, exp_avg = m, exp_avg_sq = v, step_out = t0, scaler_out = None if scaler is None else loss_scale_advance(scaler, overflow, gated), applied = not (gated or overflow))
	if not out['applied']:
		return out
	gc = gd * clip_coef(sumsq, max_norm, grad_scale, scaler)
	t = t0 + 1.0
	bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
	m = b1 * m + (1.0 - b1) * gc
	v = b2 * v + (1.0 - b2) * gc * gc
	pd = pd * (1.0 - lr * wd) - (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
	out.update(p = pd, exp_avg = m, exp_avg_sq = v, step_out = float(f32(t0) + f32(1)))
	return out


# ------------------------------------------------------------------------------------------------ NovoGrad (optimizers.py:66-90 + clip_grad_norm_)

def segment_sumsq(offsets, g):
	"""per-segment sums of squares, float64 (n_seg,); an empty segment has 0"""
	gd = f64(g)
	return torch.stack([gd[lo:hi].pow(2).sum() for lo, hi in zip(offsets[:-1], offsets[1:])])


def novograd_step(offsets, p, g, mom, ema_in, max_norm, lr, beta1, beta2, eps, weight_decay, dampening, first, loss_gate = None, grad_scale = 1.0, scaler = None, lr_dev = None):
	"""offsets: host list [n_seg + 1], segment s = elements offsets[s] .. offsets[s + 1].  ema_in: (n_seg,) or, for first < 0, (n_seg + 1,)
	with the applied-step counter behind the EMAs.
	-> dict(p, mom, ema_out (float64, n_seg), counter (float or None), g2 (n_seg), total_norm, scaler_out, applied).
	g2[s] = |g_s|^2; ema[s] = first ? g2 clip^2 : b2 ema + (1 - b2) g2 clip^2 (the EMA of the CLIPPED gradient's squared norm);
	d = g clip / sqrt(ema[s] + eps) (+ wd p when wd > 0) (x (1 - b1) with dampening); mom = first ? d : b1 mom + d; p -= lr mom.
	total_norm = sqrt(sum g2) x grad_scale / loss scale, also on a skipped step."""
	n_seg = len(offsets) - 1
	pd, gd, md, ed = f64(p), f64(g), f64(mom), f64(ema_in)
	lr = scalar(lr_dev) if lr_dev is not None else r32(lr)
	b1, b2, eps, wd = r32(beta1), r32(beta2), r32(eps), r32(weight_decay)
	g2 = segment_sumsq(offsets, g)
	total_sq = float(g2.sum())
	gated = is_gated(loss_gate)
	overflow = loss_scale_overflow(scaler, total_sq)
	counter = float(ed[n_seg]) if first < 0 else None
	out = dict(p = pd, mom = md, ema_out = ed[:n_seg], counter = counter, g2 = g2, total_norm = grad_norm(total_sq, grad_scale, scaler),
	           scaler_out = None if scaler is None else loss_scale_advance(scaler, overflow, gated), applied = not (gated or overflow))
	if not out['applied']:
		return out
	if first < 0:
		first, counter = counter == 0.0, counter_next(counter)
	clip = clip_coef(total_sq, max_norm, grad_scale, scaler)
	g2c = g2 * clip * clip
	ema = g2c if first else ed[:n_seg] * b2 + g2c * (1.0 - b2)
	inv = torch.zeros_like(pd)
	for s, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
		inv[lo:hi] = 1.0 / (ema[s] + eps).sqrt()
	d = gd * clip * inv
	if wd > 0:
		d = d + wd * pd
	if dampening:
		d = d * (1.0 - b1)
	md = d if first else md * b1 + d
	out.update(p = pd - lr * md, mom = md, ema_out = ema, counter = counter)
	return out
