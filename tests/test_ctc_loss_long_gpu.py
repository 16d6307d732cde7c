"""CTC loss and gradient past 1,023 labels and ~12,000 frames: convasr_ctc_loss_long (csrc/ctc_long.hip) against F.ctc_loss in float64
(oracle.convasr_oracle.ctc_loss, the reference's own call at models.py:323), and the routing of ops.ctc_loss up to the model's surface.

The error bars are those of test_ctc_against_oracle / test_ctc_every_split_of_the_states_over_the_two_waves (tests/test_kernels_gpu.py):
nll rtol 1e-5 / atol 1e-4, gradient rtol 1e-4 / atol 2e-4 max(1, T / 1100)^1.5, and for T > 1100 a maximum absolute gradient error no
larger than that of torch's fp32 F.ctc_loss against the same float64.  Every check prints its worst share of each bar before it asserts
(pytest -s shows them; profiles/NOTEBOOK.md records them)."""
import pytest
import torch

from oracle import convasr_oracle as O

gpu = pytest.mark.gpu


def dev():
	return torch.device('cuda:0')


def grad_atol(T):
	return 2e-4 * max(1.0, T / 1100) ** 1.5


def share(a, b, rtol, atol):
	"""worst |a - b| / (atol + rtol |b|) over all elements (<= 1: within the bar), and the largest absolute error"""
	a, b = a.detach().double().cpu(), b.detach().double().cpu()
	assert a.shape == b.shape, (a.shape, b.shape)
	if a.numel() == 0:
		return 0.0, 0.0
	err = (a - b).abs()
	return float((err / (atol + rtol * b.abs())).max()), float(err.max())


def batch(B, C, T, S, seed, scale = 1.0, repeats = True):
	torch.manual_seed(seed)
	lp = (torch.randn(B, C, T) * scale).log_softmax(dim = 1)
	y = torch.randint(0, C - 1, (B, S))
	if repeats and S > 0:
		y[-1, : S // 3] = y[-1, 0]  # no s-2 move there, and that many more frames needed
	return lp, y


def reference(lp, y, olen, ylen, fp32 = False):
	"""(nll, grad, feasible) of F.ctc_loss in float64; with fp32 also the maximum absolute gradient error of torch's fp32 F.ctc_loss over the feasible utterances"""
	lpr = lp.double().requires_grad_(True)
	ref = O.ctc_loss(lpr, y, olen, ylen)
	fin = torch.isfinite(ref)
	ref[fin].sum().backward()
	out = [ref.detach(), lpr.grad, fin]
	if fp32:
		lp32 = lp.clone().requires_grad_(True)
		r32 = O.ctc_loss(lp32, y, olen, ylen)
		r32[torch.isfinite(r32)].sum().backward()
		out.append(float((lp32.grad.double() - lpr.grad)[fin].abs().max()))
	return out


def check(what, nll, grad, ref, T, err_fp32 = None):
	"""the three bars, each share printed before anything is asserted"""
	rn, rg, fin = ref[0], ref[1], ref[2]
	s_nll, _ = share(nll.cpu()[fin], rn[fin], 1e-5, 1e-4)
	s_grad, e_grad = share(grad.cpu()[fin], rg[fin], 1e-4, grad_atol(T))
	line = f'ctc_loss_long {what}: share of the nll bar {s_nll:.3f}, of the gradient bar {s_grad:.3f} (max abs err {e_grad:.3e}, atol {grad_atol(T):.3e})'
	if err_fp32 is not None:
		line += f', of torch fp32\'s own error {e_grad / err_fp32:.4f} ({err_fp32:.3e})'
	print(line)
	assert torch.equal(torch.isfinite(nll).cpu(), fin), (what, nll, rn)
	assert s_nll <= 1.0, (what, 'nll', s_nll)
	assert s_grad <= 1.0, (what, 'grad vs float64', s_grad, e_grad)
	if err_fp32 is not None:
		assert e_grad <= err_fp32, (what, 'grad vs float64: worse than torch fp32', e_grad, err_fp32)


def ragged(B, T, S):
	"""olen / ylen as test_ctc_against_oracle draws them"""
	olen = torch.randint(max(T // 2, 2 * S + 1), T + 1, (B, ))
	olen[0] = T
	ylen = torch.randint(max(S // 2, 1), S + 1, (B, ))
	ylen[-1] = S
	return olen, ylen


@gpu
@pytest.mark.parametrize('shape', [(3, 38, 120, 1), (2, 38, 64, 31), (2, 129, 300, 40), (2, 38, 600, 200)])
def test_long_route_forced_where_the_short_kernel_also_runs(shape):
	"""one block and three states; T below a chunk; C above a wave; 401 states over two blocks -- at chunk lengths 16, 64 and the default,
	which must agree bit for bit (the renormalisation is keyed on the frame index and the block, not on the cut)"""
	from convasr_amd import ops
	B, C, T, S = shape
	lp, y = batch(B, C, T, S, T)
	olen, ylen = ragged(B, T, S)
	ref = reference(lp, y, olen, ylen)
	lpd = ops.as_cl(lp.to(dev()))
	first = None
	for chunk in (16, 64, 0):
		nll, grad = ops.ctc_loss_long(lpd, y, olen, ylen, C - 1, chunk_frames = chunk)
		check(f'{shape} chunk {chunk}', nll, grad, ref, T)
		if first is None:
			first = (nll, grad)
		assert torch.equal(nll, first[0]) and torch.equal(grad, first[1]), chunk


@gpu
@pytest.mark.parametrize('dS', [0, -1])
@pytest.mark.parametrize('dT', [-1, 0, 1])
def test_long_route_at_the_edges_of_its_tiles(dS, dT):
	"""S = SB / 2: 2 S + 1 = SB + 1 states, the last one alone in the second block; S = SB / 2 - 1: SB - 1 states; T one below, at and one
	above a chunk"""
	from convasr_amd import ops
	SB, CH = ops.ctc_loss_long_tiles()
	B, C, S, T = 2, 38, SB // 2 + dS, CH + dT
	lp, y = batch(B, C, T, S, 7 * S + T, scale = 2.0)
	olen, ylen = torch.tensor([T, T - 7]), torch.tensor([S, S])
	need = max(S + int((y[b, 1:] == y[b, :-1]).sum()) for b in range(B))
	assert need <= T - 7, (need, T)  # every utterance is feasible
	ref = reference(lp, y, olen, ylen)
	assert bool(ref[2].all())
	lpd = ops.as_cl(lp.to(dev()))
	first = None
	for chunk in (16, 0):
		nll, grad = ops.ctc_loss_long(lpd, y, olen, ylen, C - 1, chunk_frames = chunk)
		check(f'S {S} T {T} chunk {chunk}', nll, grad, ref, T)
		if first is None:
			first = (nll, grad)
		assert torch.equal(nll, first[0]) and torch.equal(grad, first[1]), chunk


@gpu
@pytest.mark.parametrize('shape', [(2, 38, 2100, 1024), (2, 38, 2600, 1100), (1, 129, 4200, 2047), (2, 38, 13000, 600)])
def test_past_the_short_kernel_through_ops_ctc_loss(shape):
	"""the first label count over the short kernel's limit (2,049 states), beyond it, 4,095 states, and frames past its LDS slots with the
	labels inside them: ops.ctc_loss routes all four to the tiled kernel"""
	from convasr_amd import ops, _lib
	B, C, T, S = shape
	assert not _lib.load().convasr_ctc_loss_supported(B, T, C, S)
	lp, y = batch(B, C, T, S, S, scale = 2.0)
	olen, ylen = torch.tensor([T, T - 7][:B]), torch.full((B, ), S)
	ref = reference(lp, y, olen, ylen, fp32 = True)
	assert bool(ref[2].all())
	nll, grad = ops.ctc_loss(ops.as_cl(lp.to(dev())), y, olen, ylen, C - 1)
	check(f'{shape}', nll, grad, ref, T, err_fp32 = ref[3])
	assert float(grad[-1, :, int(olen[-1]):].abs().sum()) == 0.0


@gpu
def test_ragged_and_degenerate_utterances_in_one_long_batch():
	from convasr_amd import ops
	B, C, T, S = 5, 38, 2600, 1100
	lp, y = batch(B, C, T, S, 4, scale = 2.0)
	olen = torch.tensor([T, T, 300, 900, T - 1])
	ylen = torch.tensor([S, 0, 100, 1000, S])
	ref = reference(lp, y, olen, ylen, fp32 = True)
	assert ref[2].tolist() == [True, True, True, False, True]
	nll, grad = ops.ctc_loss(ops.as_cl(lp.to(dev())), y, olen, ylen, C - 1)
	check('ragged batch', nll, grad, ref, T, err_fp32 = ref[3])
	assert torch.isinf(nll[3]) and nll[3] > 0 and float(grad[3].abs().max()) == 0.0  # infeasible: +inf, a zero gradient
	assert not torch.isnan(grad).any() and not torch.isnan(nll).any()
	for b in range(B):
		assert float(grad[b, :, int(olen[b]):].abs().sum()) == 0.0, b


@gpu
def test_infinite_and_nan_log_probs_on_the_long_route():
	from convasr_amd import ops
	B, C, T, S = 3, 38, 2100, 1024
	torch.manual_seed(1)
	lp = torch.randn(B, C, T).log_softmax(dim = 1)
	y = torch.randint(0, C - 2, (B, S))  # class C - 2 never occurs in a target
	for b in range(B):  # consecutive equal labels removed, as in test_ctc_infinite_and_nan_log_probs
		for i in range(1, S):
			if y[b, i] == y[b, i - 1]:
				y[b, i] = (y[b, i] + 1) % (C - 2)
	lp[0, C - 2] = -float('inf')
	lp[1, int(y[1, 1000]), :] = -float('inf')
	olen, ylen = torch.full((B, ), T), torch.full((B, ), S)
	ref = reference(lp, y, olen, ylen)
	assert ref[2].tolist() == [True, False, True]
	nll, grad = ops.ctc_loss(ops.as_cl(lp.to(dev())), y, olen, ylen, C - 1)
	assert torch.isinf(nll[1]) and nll[1] > 0 and float(grad[1].abs().max()) == 0.0
	keep = torch.ones(C, dtype = torch.bool)
	keep[C - 2] = False
	s_nll, _ = share(nll.cpu()[[0, 2]], ref[0][[0, 2]], 1e-5, 1e-4)
	s_g0, _ = share(grad.cpu()[0][keep], ref[1][0][keep], 1e-4, grad_atol(T))
	s_g2, _ = share(grad.cpu()[2], ref[1][2], 1e-4, grad_atol(T))
	print(f'ctc_loss_long -inf log-probs: share of the nll bar {s_nll:.3f}, of the gradient bar {s_g0:.3f} beside a forbidden class, {s_g2:.3f} on a clean utterance')
	assert torch.isfinite(nll[0]) and torch.isfinite(nll[2])
	assert s_nll <= 1.0 and s_g0 <= 1.0 and s_g2 <= 1.0, (s_nll, s_g0, s_g2)
	lp[2, :, 100] = float('nan')  # what log_softmax makes of a frame with a NaN logit
	nll, grad = ops.ctc_loss(ops.as_cl(lp.to(dev())), y, olen, ylen, C - 1)  # returns
	torch.cuda.synchronize()
	assert not torch.isfinite(nll[2]) and torch.isfinite(nll[0]) and torch.isinf(nll[1])


@gpu
@pytest.mark.parametrize('shape', [(2, 38, 2600, 1100), (4, 38, 700, 200)])
def test_long_route_launches_are_bitwise_identical(shape):
	"""every value a tile reads was written by an earlier launch and the gradient adds in a fixed order: nothing depends on timing, which a
	memory-bound kernel on a second stream perturbs"""
	from convasr_amd import ops
	B, C, T, S = shape
	d = dev()
	lp, y = batch(B, C, T, S, S, scale = 2.0)
	lpd = ops.as_cl(lp.to(d))
	olen, ylen = torch.tensor([T, T - 7] * (B // 2), device = d), torch.full((B, ), S, device = d)
	y = y.to(d)
	nll0, g0 = ops.ctc_loss_long(lpd, y, olen, ylen, C - 1)
	assert torch.isfinite(nll0).all()
	side, junk = torch.cuda.Stream(), torch.empty(32 << 20, device = d)
	for i in range(3):
		with torch.cuda.stream(side):
			junk.add_(1.0)
		nll, g = ops.ctc_loss_long(lpd, y, olen, ylen, C - 1)
		assert torch.equal(nll, nll0) and torch.equal(g, g0), i
	torch.cuda.synchronize()


@gpu
def test_functional_ctc_loss_backward_past_the_short_kernel():
	"""functional.ctc_loss with norm = ylen: backward of a weighted sum is grad * g / norm, against float64 autograd on the oracle"""
	from convasr_amd import functional as Fn
	B, C, T, S = 2, 38, 2100, 1024
	d = dev()
	lp, y = batch(B, C, T, S, 11, scale = 2.0)
	olen, ylen = torch.tensor([T, T - 7]), torch.full((B, ), S)
	w = torch.tensor([0.75, 1.5])
	lpr = lp.double().requires_grad_(True)
	ref = O.ctc_loss(lpr, y, olen, ylen) / ylen
	assert torch.isfinite(ref).all()
	(ref * w.double()).sum().backward()
	lpd = lp.to(d).requires_grad_(True)
	loss = Fn.ctc_loss(lpd, y.to(d), olen.to(d), ylen.to(d), C - 1, norm = ylen.to(d))
	(loss * w.to(d)).sum().backward()
	s_nll, _ = share(loss, ref, 1e-5, 1e-4)
	s_grad, e_grad = share(lpd.grad, lpr.grad, 1e-4, grad_atol(T))
	print(f'functional.ctc_loss {(B, C, T, S)}: share of the nll bar {s_nll:.3f}, of the gradient bar {s_grad:.3f} (max abs err {e_grad:.3e})')
	assert s_nll <= 1.0 and s_grad <= 1.0, (s_nll, s_grad)


@gpu
def test_model_loss_on_45_seconds_against_1100_labels():
	"""JasperNet.forward with targets on an unsegmented utterance: the tiny configuration of SURVEY.md on 4,500 feature frames (45 s), 2,250
	output frames against 1,100 labels"""
	import convasr_amd as ca
	from convasr_amd import _lib
	d = dev()
	torch.manual_seed(3)
	model = ca.models.JasperNet(64, [38], dropouts = [0.0], dropout = 0, check_time_dim_padded = False, **O.TINY).to(d).train()
	B, F, S = 2, 4500, 1100
	x, xlen = torch.randn(B, 64, F, device = d), torch.tensor([1.0, 0.95], device = d)
	y, ylen = torch.randint(0, 37, (B, 1, S), device = d), torch.full((B, 1), S, device = d)
	out = model(x, xlen, y, ylen)
	lp, olen, loss = out['log_probs'][0], out['olen'][0], out['loss']
	assert lp.shape[-1] > 2200 and not _lib.load().convasr_ctc_loss_supported(B, lp.shape[-1], lp.shape[1], S)
	assert torch.isfinite(loss).all()
	ref = O.ctc_loss(lp.detach().double().cpu(), y[:, 0].cpu(), olen.cpu(), ylen[:, 0].cpu()) / ylen[:, 0].cpu()
	s_nll, _ = share(loss, ref, 1e-5, 1e-4)
	print(f'JasperNet loss at {tuple(lp.shape)}: share of the nll bar {s_nll:.3f}')
	assert s_nll <= 1.0, s_nll
	loss.sum().backward()
	g = model.backbone[0].conv[0][-1].weight.grad
	assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


@gpu
def test_long_route_guards():
	from convasr_amd import ops, _lib
	B, C, T, S = 2, 38, 2100, 1024
	d = dev()
	lp, y = batch(B, C, T, S, 5)
	olen, ylen = torch.tensor([T, T - 7], device = d), torch.full((B, ), S, device = d)
	lpd, yd = ops.as_cl(lp.to(d)), y.to(d)
	need = _lib.load().convasr_ctc_loss_long_workspace_bytes(B, T, C, S)
	with pytest.raises(_lib.ConvasrHipError, match = str(need)):
		ops.ctc_loss_long(lpd, yd, olen, ylen, C - 1, workspace_cap = 1 << 20)
	with pytest.raises(_lib.ConvasrHipError):
		ops.ctc_loss_long(lp.permute(0, 2, 1).contiguous().permute(0, 2, 1), y, olen.cpu(), ylen.cpu(), C - 1)  # a CPU tensor: before any launch
	graph = torch.cuda.CUDAGraph()
	with pytest.raises(_lib.ConvasrHipError, match = 'captured'):
		with torch.cuda.graph(graph):
			ops.ctc_loss(lpd, yd, olen, ylen, C - 1)
	assert not torch.cuda.is_current_stream_capturing()  # (the graph is never replayed)
	nll, _ = ops.ctc_loss(lpd, yd, olen, ylen, C - 1, need_grad = False)  # forward only, and the stream is usable again
	assert torch.isfinite(nll).all()


@gpu
def test_short_route_is_untouched_by_the_routing():
	"""a shape the short kernel takes goes to it exactly as before: bit-equal to a direct convasr_ctc_loss call"""
	from convasr_amd import ops, _lib
	B, C, T, S = 8, 38, 753, 150
	d = dev()
	lp, y = batch(B, C, T, S, 9)
	olen, ylen = ragged(B, T, S)
	lpd, yd, od, yl = ops.as_cl(lp.to(d)), y.to(d), olen.to(d), ylen.to(d)
	assert _lib.load().convasr_ctc_loss_supported(B, T, C, S)
	nll, grad = ops.ctc_loss(lpd, yd, od, yl, C - 1)
	nll, grad = nll.clone(), grad.clone()
	ws = torch.empty(_lib.load().convasr_ctc_workspace_bytes(B, T, S), dtype = torch.uint8, device = d)
	nll2, grad2 = torch.empty(B, device = d), ops.empty_cl(B, C, T, torch.float32, d)
	_lib.call('convasr_ctc_loss', _lib.ptr(lpd), _lib.ptr(yd), _lib.ptr(od), _lib.ptr(yl), _lib.ptr(nll2), _lib.ptr(grad2), _lib.ptr(ws), B, T, C, S, C - 1, _lib.stream_ptr())
	assert torch.equal(nll, nll2) and torch.equal(grad, grad2)
	assert torch.isfinite(nll).all()
