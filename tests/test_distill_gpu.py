"""Distillation on the MI355X: ops.topk_frames (exact) and ops.distill_kl (against the float64 restatement, tests/_distill_ref.py) on both
sides of their two mappings and around the row mapping's 128-frame workgroup; functional.distill_loss under autograd; train_step with a
teacher against torch autograd of F.ctc_loss + F.kl_div on the model's own forward; evaluate_model's saved top-k logits and the
TeacherStore round trip.

Bars, each printed next to what was measured (R.held): per-frame tau^2 KL and kd[b] on the project's entropy bar, rtol 1e-4 + atol 1e-5
(kd[b]: the atol times the utterance's frames); the gradient on tau times the log-softmax-backward bar, rtol 1e-4 + atol 1e-5; top-k exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _distill_ref as R

pytestmark = pytest.mark.gpu
TORCH = dict(float32 = torch.float32, float16 = torch.float16, uint8 = torch.uint8, int16 = torch.int16, int32 = torch.int32)
ALPHABET = 'абвгдеёжзийклмнопрстуфхцчшщъыьэюя'


def _dev():
	return torch.device('cuda:0')


def _to_dev(x):
	"""(B, T, C) numpy -> the (B, C, T) channels-last device tensor a model hands over."""
	return torch.from_numpy(np.ascontiguousarray(x)).to(_dev()).permute(0, 2, 1)


def _btk(t):
	"""A (B, k, T) result -> (B, T, k) numpy."""
	return t.permute(0, 2, 1).cpu().numpy()


def _bits(t):
	return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
	"""Bit-equal, a NaN equal to any NaN."""
	if a.is_floating_point():
		nan = torch.isnan(a)
		return a.dtype == b.dtype and a.shape == b.shape and torch.equal(nan, torch.isnan(b)) and torch.equal(_bits(a)[~nan], _bits(b)[~nan])
	return a.dtype == b.dtype and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ top-k

@pytest.mark.parametrize('C', R.CLASSES)
def test_topk_frames_is_exact(C):
	from convasr_amd import ops, models
	assert ops.frame_uncertainty_row_classes() == 64 and ops.topk_frames_max_k() == 32
	for T in R.FRAMES:
		for name, x in R.topk_inputs(C, T).items():
			xd = _to_dev(x)
			assert ops.is_cl(xd)
			for k in sorted({1, min(5, C), min(C, 32)}):
				want_v, want_i = R.topk(x, k)
				values, indices = ops.topk_frames(xd, k)
				assert values.shape == (R.B, k, T) and indices.shape == (R.B, k, T) and values.dtype == torch.float32 and indices.dtype == torch.int32
				assert values.permute(0, 2, 1).is_contiguous() and indices.permute(0, 2, 1).is_contiguous()  # (B, T, k) memory
				what = f'C {C} T {T} {name} k {k}'
				assert np.array_equal(_btk(indices), want_i), what
				assert _same(values.permute(0, 2, 1).cpu(), torch.from_numpy(want_v)), what
				if name in R.TIE_FREE:
					top = torch.topk(xd, k, dim = 1)
					assert torch.equal(top.values, values) and torch.equal(top.indices, indices.long()), what
			# the storage types, two runs, a channels-first input, the models surface: at the largest k
			k = min(C, 32)
			values, indices = ops.topk_frames(xd, k)
			for vdt in (torch.float32, torch.float16):
				for idt in ((torch.uint8, ) if C <= 256 else ()) + (torch.int16, torch.int32):
					v, i = ops.topk_frames(xd, k, vdt, idt)
					assert v.dtype == vdt and i.dtype == idt and torch.equal(i.long(), indices.long()) and _same(v, values.to(vdt)), (name, vdt, idt)
					assert _same(v.cpu(), torch.from_numpy(want_v.astype(np.float16 if vdt == torch.float16 else np.float32)).permute(0, 2, 1))
					v2, i2 = ops.topk_frames(xd, k, vdt, idt)
					assert _same(v, v2) and torch.equal(i, i2)
			first = xd.contiguous()  # torch-contiguous (B, C, T): the op converts it
			assert not ops.is_cl(first) or T == 1
			v, i = ops.topk_frames(first, k)
			assert _same(v, values) and torch.equal(i, indices)
			if name in R.TIE_FREE:
				saved = models.sparse_topk(xd, k, dim = 1, fill_value = -7.0)
				assert saved['indices'].dtype == torch.int64 and saved['values'].dtype == torch.float32 and saved['shape'] == xd.shape
				top = torch.topk(xd, k, dim = 1)
				assert torch.equal(models.sparse_topk_todense(saved), torch.full_like(xd, -7.0).scatter_(1, top.indices, top.values))
				small = models.sparse_topk(xd, k, dim = -2, indices_dtype = torch.int16, values_dtype = torch.float16)
				assert small['indices'].dtype == torch.int16 and torch.equal(models.sparse_topk_todense(small), torch.zeros_like(xd).scatter_(1, top.indices, top.values.half().float()))


@pytest.mark.parametrize('C', [2048, 2049, 4097, 8192])
def test_topk_frames_on_wide_rows(C):
	"""The wave mapping keeps a workgroup's keys in 32 KiB of LDS: four frames a workgroup up to 2,048 classes, two up to 4,096, one above."""
	from convasr_amd import ops
	rng = np.random.default_rng(C)
	x = rng.integers(-30, 31, (2, 5, C)).astype(np.float32)  # tied
	x[0, 1, rng.integers(0, C, 3)] = np.nan
	xd = _to_dev(x)
	for k in (1, 32):
		want_v, want_i = R.topk(x, k)
		values, indices = ops.topk_frames(xd, k, indices_dtype = torch.int16)
		assert np.array_equal(_btk(indices), want_i) and _same(values.permute(0, 2, 1).cpu(), torch.from_numpy(want_v))
	z, teacher = ((rng.standard_normal((2, 5, C)) * 3).astype(np.float32) for _ in range(2))
	values, indices = ops.topk_frames(_to_dev(teacher), 32, torch.float16, torch.int16)
	res = ops.distill_kl(_to_dev(z), values, indices, torch.tensor([5, 3]), 2.0, per_frame = True)
	R.check_distill(f'C {C}', _got(res), R.distill(z, _btk(values), _btk(indices), [5, 3], 2.0), [5, 3], 2.0, 5)


def test_topk_frames_refuses_what_is_outside_its_envelope():
	from convasr_amd import ops, _lib
	x5, x64, x257 = (torch.randn(2, 9, C, device = _dev()).permute(0, 2, 1) for C in (5, 64, 257))
	for x, kw in ((x5, dict(k = 0)), (x5, dict(k = 6)), (x64, dict(k = 33)), (x257, dict(k = 2, indices_dtype = torch.uint8)), (x5, dict(k = 2, indices_dtype = torch.int64)), (x5, dict(k = 2, values_dtype = torch.bfloat16))):
		with pytest.raises(_lib.ConvasrHipError):
			ops.topk_frames(x, **kw)
	with pytest.raises(_lib.ConvasrHipError):
		ops.topk_frames(x5.cpu(), 2)
	assert ops.topk_frames(x257, 2, indices_dtype = torch.int16)[1].dtype == torch.int16 and ops.topk_frames(x64, 32)[0].shape == (2, 32, 9)


# ------------------------------------------------------------------------------------------------ KL and gradient

def _got(res):
	kd, grad, frames = res
	return kd.cpu().numpy(), frames.cpu().numpy(), grad.permute(0, 2, 1).cpu().numpy()


@pytest.mark.parametrize('C', R.CLASSES)
def test_distill_kl_against_the_float64_restatement(C):
	from convasr_amd import ops
	worst = 0.0
	for T in R.FRAMES:
		teacher = _to_dev(R.distill_teacher_logits(C, T))
		for name, z in R.distill_students(C, T).items():
			zd = _to_dev(z)
			for k, tau, vdt, idt in R.distill_settings(C):
				values, indices = ops.topk_frames(teacher, k, TORCH[vdt], TORCH[idt])  # the teacher as it would be stored
				v_np, i_np = _btk(values), _btk(indices)
				for lengths in R.lengths_of(T):
					what = f'C {C} T {T} {name} k {k} tau {tau} {vdt} {idt} lengths {lengths}'
					res = ops.distill_kl(zd, values, indices, torch.tensor(lengths), tau, per_frame = True)
					kd, grad, frames = res
					assert kd.shape == (R.B, ) and frames.shape == (R.B, T) and grad.shape == zd.shape and ops.is_cl(grad) and grad.dtype == torch.float32
					want = R.distill(z, v_np, i_np, lengths, tau)
					print(what)
					worst = max(worst, R.check_distill(what, _got(res), want, lengths, tau, T))
					for b, n in enumerate(lengths):
						assert not grad[b, :, n:].any() and not frames[b, n:].any(), what  # exactly 0 past the lengths
						assert n > 0 or float(kd[b]) == 0.0, what
			# at the last setting: two runs, without the gradient, int64 indices, a channels-first student
			again = ops.distill_kl(zd, values, indices, torch.tensor(lengths), tau, per_frame = True)
			assert all(_same(a, b) for a, b in zip(res, again))
			kd_only, none = ops.distill_kl(zd, values, indices, torch.tensor(lengths), tau, need_grad = False)
			assert none is None and _same(kd_only, kd)
			wide = ops.distill_kl(zd.contiguous(), values.float(), indices.long(), torch.tensor(lengths, device = _dev()), tau)
			assert _same(wide[0], kd) and _same(wide[1], grad)
	print(f'C {C}: at most {worst:.3f} of a bar')


def test_distill_kl_student_equal_to_the_teacher_and_an_out_of_range_index():
	from convasr_amd import ops, _lib
	rng = np.random.default_rng(2)
	T, C = 129, 32
	z = (rng.standard_normal((R.B, T, C)) * 3).astype(np.float32)
	zd = _to_dev(z)
	for tau in R.TAUS:
		values, indices = ops.topk_frames(zd, C)  # k = C: the whole teacher, and the student is the teacher
		kd, grad, frames = ops.distill_kl(zd, values, indices, torch.tensor([T, T - 1, 0]), tau, per_frame = True)
		print(f'tau {tau}: |kd| {kd.abs().max().item():.3e}, per frame {frames.abs().max().item():.3e}, gradient {grad.abs().max().item():.3e}')
		assert float(frames.abs().max()) <= R.KD_BAR[1] and float(kd.abs().max()) <= R.KD_BAR[1] * T and float(grad.abs().max()) <= tau * R.GRAD_BAR[1]
	values, indices = ops.topk_frames(_to_dev(rng.standard_normal((R.B, T, C)).astype(np.float32)), 8, torch.float16, torch.int16)
	lengths = torch.tensor([T, T, T])
	clean = ops.distill_kl(zd, values, indices, lengths, 2.0, per_frame = True)
	for wrong in (C, -1):
		poked = indices.clone()
		poked[1, 3, 77] = wrong
		kd, grad, frames = ops.distill_kl(zd, values, poked, lengths, 2.0, per_frame = True)
		hit = torch.zeros(R.B, T, dtype = torch.bool, device = _dev())
		hit[1, 77] = True
		assert torch.equal(torch.isnan(frames), hit) and torch.equal(torch.isnan(grad).all(1), hit) and torch.equal(torch.isnan(grad).any(1), hit)
		assert _same(frames[~hit], clean[2][~hit]) and _same(grad.permute(0, 2, 1)[~hit], clean[1].permute(0, 2, 1)[~hit])
		assert bool(torch.isnan(kd[1])) and _same(kd[[0, 2]], clean[0][[0, 2]])
	for kw in (dict(temperature = 0.0), dict(temperature = -1.0)):
		with pytest.raises(_lib.ConvasrHipError):
			ops.distill_kl(zd, values, indices, lengths, **kw)
	with pytest.raises(ValueError):
		ops.distill_kl(zd, values[:, :, 1:], indices[:, :, 1:], lengths)


def _kd_autograd(logits, values, indices, olen, tau):
	"""float64 torch autograd: tau^2 * F.kl_div(log_softmax(z / tau), p_dense, reduction = 'sum') per utterance, over its own frames;
	logits (B, C, T) with or without a graph, values / indices (B, k, T)."""
	C = logits.shape[1]
	dense = torch.from_numpy(R.dense_teacher(_btk(values), _btk(indices), C, tau)).to(logits.device)  # (B, T, C)
	lq = F.log_softmax(logits.double().permute(0, 2, 1) / tau, dim = -1)
	return torch.stack([tau * tau * F.kl_div(lq[b, :n], dense[b, :n], reduction = 'sum') for b, n in enumerate(olen.tolist())])


@pytest.mark.parametrize('C, k', [(38, 8), (130, 5)])
def test_distill_loss_under_autograd(C, k):
	from convasr_amd import functional as Fn, models
	rng = np.random.default_rng(C)
	T, tau = 131, 2.0
	teacher = models.sparse_topk(_to_dev((rng.standard_normal((R.B, T, C)) * 3).astype(np.float32)), k, dim = 1, indices_dtype = torch.uint8, values_dtype = torch.float16)
	olen = torch.tensor([T, 60, 1], device = _dev())
	g = torch.tensor([0.5, -2.0, 3.0], device = _dev())
	z = _to_dev((rng.standard_normal((R.B, T, C)) * 3).astype(np.float32))
	leaf = z.clone().requires_grad_(True)
	kd = Fn.distill_loss(leaf, teacher, olen, tau)
	kd.backward(g)
	ref = z.clone().requires_grad_(True)
	want = _kd_autograd(ref, teacher['values'], teacher['indices'], olen, tau)
	want.backward(g.double())
	print(f'C {C} k {k}')
	R.held('kd', kd.detach().cpu().numpy(), want.detach().cpu().numpy(), R.KD_BAR[0], R.KD_BAR[1] * olen.cpu().numpy())
	scale = g.abs().cpu().numpy()[:, None, None]
	R.held('d kd / d logits x g', leaf.grad.cpu().numpy(), ref.grad.cpu().numpy(), R.GRAD_BAR[0], tau * R.GRAD_BAR[1] * np.broadcast_to(scale, tuple(z.shape)))
	pair = Fn.distill_loss(z, (teacher['values'], teacher['indices']), olen, tau)  # a (values, indices) pair, no graph
	assert torch.equal(pair, kd.detach()) and not pair.requires_grad


# ------------------------------------------------------------------------------------------------ the step

def _tiny(seed):
	"""The tiny model of tests/test_models_gpu.py (dropout 0.2, one block), fp32."""
	import convasr_amd as ca
	torch.manual_seed(seed)
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	return ca.models.JasperNet(64, [38], base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, frontend = fe,
		check_time_dim_padded = False, nonlinearity = ('hardtanh', 0, 20), dilation = 2).to(_dev())


def _two_utterances():
	g = torch.Generator().manual_seed(11)
	d = _dev()
	x = (torch.rand(2, 16000, generator = g) * 2 - 1).to(d)
	return x, torch.tensor([1.0, 0.7], device = d), torch.randint(0, 37, (2, 1, 12), generator = g).to(d), torch.tensor([[12], [7]], device = d)


def _student(lr = 1.0):
	import convasr_amd as ca
	model = _tiny(1).train()
	flat = ca.train.FlatParameters(model)
	return model, flat, ca.train.SGD(flat, lr = lr, momentum = 0.0, weight_decay = 0.0)


def _step(model, opt, batch, **kw):
	import convasr_amd as ca
	ca.functional.manual_seed(7)  # the same dropout masks in every step of this file
	return ca.train.train_step(model, opt, *batch, max_norm = 1e9, **kw)


def test_train_step_with_a_teacher_matches_torch_autograd_of_ctc_plus_kl():
	import convasr_amd as ca
	from convasr_amd import distill, functional as Fn
	batch = _two_utterances()
	x, xlen, y, ylen = batch
	weight, tau = 0.5, 2.0
	teacher_model = _tiny(2).train()
	teacher, t_olen = distill.teacher_from_model(teacher_model, x, xlen, 8)
	assert teacher_model.training and teacher['values'].dtype == torch.float16 and teacher['indices'].dtype == torch.uint8 and teacher['values'].shape[:2] == (2, 8)
	model, flat, opt = _student()
	# the reference: the same loss composed by torch on the model's own forward, through torch autograd into the model's own backward
	Fn.manual_seed(7)
	Fn.begin_step(x.device)
	out = model(x, xlen, y = y, ylen = ylen)
	logits, olen = out['logits'][0], out['olen'][0]
	assert torch.equal(olen, t_olen)
	lp = F.log_softmax(logits.double(), dim = 1)
	ctc = F.ctc_loss(lp.permute(2, 0, 1), y[:, 0], olen, ylen[:, 0], blank = logits.shape[1] - 1, reduction = 'none')
	kd_ref = _kd_autograd(logits, teacher['values'], teacher['indices'], olen, tau)
	(ctc.mean() + weight * kd_ref.mean()).backward()
	Fn.join_side_streams()
	flat.finalize_grads()
	want = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
	opt.zero_grad()
	before = {n: p.detach().clone() for n, p in model.named_parameters()}
	res = _step(model, opt, batch, teacher = teacher, distill_weight = weight, distill_temperature = tau)
	assert not bool(res['skipped'])
	R.held('distill = mean(kd)', res['distill'].cpu().numpy(), kd_ref.mean().detach().cpu().numpy(), *R.KD_BAR[:1], R.KD_BAR[1] * float(olen.max()))
	assert res['distill'].ndim == 0 and res['distill'].is_cuda
	some = 0
	for n, p in model.named_parameters():
		if n in want and float(want[n].abs().max()) > 0:
			got = (before[n] - p.detach()).double()  # lr = 1, no momentum, no decay, no clipping: the step IS the gradient
			ref = want[n].double()
			err, tol = (got - ref).abs(), 1e-3 * float(ref.abs().max()) + 5e-3 * ref.abs()  # the tiny-model gradient bar of tests/test_models_gpu.py
			print(f'  {n}: worst error {float(err.max()):.3e}, {float((err / tol).max()):.3f} of its bar')
			assert bool((err <= tol).all()), n
			some += 1
	assert some >= 4
	# the KL term is in there: without it the decoder's gradient is another one
	model2, flat2, opt2 = _student()
	before2 = {n: p.detach().clone() for n, p in model2.named_parameters()}
	_step(model2, opt2, batch)
	n = 'decoder.0.weight'
	plain = before2[n] - dict(model2.named_parameters())[n].detach()
	assert float((plain - want[n]).abs().max()) > 10 * 1e-3 * float(want[n].abs().max())


def test_train_step_weight_zero_no_teacher_and_a_nan_teacher():
	from convasr_amd import distill
	batch = _two_utterances()
	x, xlen, y, ylen = batch
	teacher, _ = distill.teacher_from_model(_tiny(2), x, xlen, 8)
	runs = {}
	for name, kw in (('old arguments', None), ('no teacher', dict(teacher = None, distill_weight = 0.5, distill_temperature = 2.0)), ('weight 0', dict(teacher = teacher, distill_weight = 0.0, distill_temperature = 2.0))):
		model, flat, opt = _student(lr = 1e-2)
		res = _step(model, opt, batch, **(kw or {}))
		runs[name] = (flat.data.clone(), res)
	assert torch.equal(runs['old arguments'][0], runs['no teacher'][0]) and 'distill' not in runs['no teacher'][1] and sorted(runs['no teacher'][1]) == sorted(runs['old arguments'][1])
	assert torch.equal(runs['old arguments'][0], runs['weight 0'][0]) and bool(torch.isfinite(runs['weight 0'][1]['distill']))
	for device_gate in (True, False):
		model, flat, opt = _student(lr = 1e-2)
		start = flat.data.clone()
		bad = dict(teacher, values = teacher['values'].clone())
		bad['values'][1, 0, 3] = float('nan')
		res = _step(model, opt, batch, teacher = bad, distill_weight = 0.5, device_gate = device_gate)
		assert bool(res['skipped']) and torch.equal(flat.data, start) and not bool(torch.isfinite(res['distill'])) and bool(torch.isfinite(res['loss_cur']))


def test_train_epoch_hands_the_teacher_on_and_refuses_graphs():
	import convasr_amd as ca
	from convasr_amd import distill
	batch = _two_utterances()
	teacher_model = _tiny(2)
	seen = []

	def teacher_fn(b):
		seen.append(b[0])
		return distill.teacher_from_model(teacher_model, b[2], b[3], 4)[0]

	model, flat, opt = _student(lr = 1e-2)
	got = []
	it = ca.train.train_epoch(model, opt, [(['meta'], None, *batch)], teacher_fn = teacher_fn, distill_weight = 0.3, distill_temperature = 2.0, on_step = lambda i, b, res: got.append(res))
	assert it == 1 and seen == [['meta']] and 'distill' in got[0] and bool(torch.isfinite(got[0]['distill']))
	with pytest.raises(ValueError):
		ca.train.train_epoch(model, opt, [], graphs = object(), teacher_fn = teacher_fn)


# ------------------------------------------------------------------------------------------------ saving

def test_evaluate_model_saves_topk_logits_and_a_teacher_store_feeds_the_step(tmp_path):
	import convasr_amd as ca
	from convasr_amd import distill
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	tok = CharTokenizerLegacy(ALPHABET)
	d = _dev()
	g = torch.Generator().manual_seed(4)
	batches = []
	for i in range(2):
		x = (torch.rand(2, 16000 + 4000 * i, generator = g) * 2 - 1).to(d)
		batches.append(([dict(example_id = 10 * i + j) for j in range(2)], None, x, torch.tensor([1.0, 0.6 + 0.1 * i], device = d), torch.randint(0, 37, (2, 1, 9), generator = g).to(d), torch.tensor([[9], [5]], device = d)))
	teacher_model = _tiny(2).train()
	plain = ca.train.evaluate_model(teacher_model, batches, tok)
	res = ca.train.evaluate_model(teacher_model, batches, tok, logits_topk = 5)
	assert teacher_model.training
	assert {k: v for k, v in res.items() if k != 'utterances'} == {k: v for k, v in plain.items() if k != 'utterances'}
	assert sorted(res['utterances']) == sorted(list(plain['utterances']) + ['logits']) and all(torch.equal(res['utterances'][k], v) for k, v in plain['utterances'].items())
	saved = res['utterances']['logits']
	assert len(saved) == 4
	teacher_model.eval()
	store = distill.TeacherStore()
	with torch.no_grad():
		for i, (meta, _, x, xlen, y, ylen) in enumerate(batches):
			out = teacher_model(x, xlen)
			for j, n in enumerate(out['olen'][0].tolist()):
				u = saved[2 * i + j]
				top = torch.topk(out['logits'][0][j, :, :n].float(), 5, dim = 0)  # of the utterance's own unpadded logits
				assert u['values'].shape == (5, n) and u['indices'].shape == (5, n) and u['values'].dtype == torch.float16 and u['indices'].dtype == torch.uint8
				assert torch.equal(u['values'], top.values.half().cpu()) and torch.equal(u['indices'].long(), top.indices.cpu())
			store.add_utterances(meta, saved[2 * i:2 * i + 2])
	teacher_model.train()
	path = str(tmp_path / 'teacher.pt')
	store.save(path)
	store = distill.TeacherStore.load(path, d)
	meta, _, x, xlen, y, ylen = batches[1]
	online, olen = distill.teacher_from_model(teacher_model, x, xlen, 5)
	T = online['values'].shape[2]
	stored = store.batch(meta, T, olen = olen)
	with pytest.raises(ValueError):
		store.batch(meta, T, olen = olen - 1)
	values = {}
	for name, teacher in (('online', online), ('stored', stored)):
		model, flat, opt = _student(lr = 1e-2)
		values[name] = _step(model, opt, (x, xlen, y, ylen), teacher = teacher, distill_weight = 0.5, distill_temperature = 2.0)['distill']
	# the restatement on the student's logits of that very step and the stored fp16 values
	model, flat, opt = _student()
	ca.functional.manual_seed(7)
	ca.functional.begin_step(d)
	z = model(x, xlen, y = y, ylen = ylen)['logits'][0].detach()  # (in training mode, with the graph: the forward the step runs)
	want =R.distill(_btk(z), _btk(stored[0]), _btk(stored[1]), olen.tolist(), 2.0)[0]
	n = np.asarray(olen.tolist(), dtype = np.float64)
	print(f"distill: online {float(values['online']):.6f}, stored {float(values['stored']):.6f}, restatement {want.mean():.6f}")
	for name in values:
		R.held(name + ' against the restatement', values[name].cpu().numpy(), want.mean(), R.KD_BAR[0], R.KD_BAR[1] * n.max())
