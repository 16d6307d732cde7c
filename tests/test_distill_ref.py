"""tests/_distill_ref.py, the float64 restatement of convasr_topk_frames / convasr_distill_kl, against independent arithmetic: torch.topk and
a brute-force sort for the order, float64 torch autograd of F.kl_div for the KL and its gradient, the full KL at k = C; and a float32 copy
of the restatement held to the GPU tests' bars on every input those tests use, so that inputs and bars are known to fit before a GPU is
involved.  No GPU needed."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _distill_ref as R


@pytest.mark.parametrize('C, k', [(2, 1), (2, 2), (38, 5), (64, 32), (65, 8), (130, 32)])
def test_topk_equals_torch_topk_on_tie_free_frames(C, k):
	rng = np.random.default_rng(C * 100 + k)
	x = rng.permuted(np.tile(np.linspace(-9.0, 9.0, C), (2, 17, 1)), axis = -1)  # a seeded permutation of distinct values per frame
	values, indices = R.topk(x, k)
	want = torch.topk(torch.from_numpy(x), k, dim = -1)
	assert np.array_equal(values, want.values.numpy()) and np.array_equal(indices, want.indices.numpy())


def _brute(row, k):
	def cmp(i, j):
		v, w = row[i], row[j]
		if np.isnan(v) or np.isnan(w):
			if np.isnan(v) and np.isnan(w):
				return i - j
			return -1 if np.isnan(v) else 1
		if v != w:
			return -1 if v > w else 1
		return i - j
	return sorted(range(len(row)), key = functools.cmp_to_key(cmp))[:k]


@pytest.mark.parametrize('C, k', [(2, 2), (7, 7), (38, 5), (65, 32)])
def test_topk_equals_a_brute_force_sort_on_ties_and_nans(C, k):
	rng = np.random.default_rng(C)
	x = rng.integers(-3, 4, (2, 9, C)).astype(np.float32)  # integer logits in -3 .. 3
	x[0, 0, :2] = [0.0, -0.0]
	x[1, 1, rng.integers(0, C, 3)] = np.nan
	x[1, 2] = np.nan
	values, indices = R.topk(x, k)
	for b in range(2):
		for t in range(9):
			want = _brute(x[b, t], k)
			assert indices[b, t].tolist() == want, (b, t)
			assert np.array_equal(values[b, t].view(np.int32), x[b, t][want].view(np.int32))
	first = R.order(x)[0, 0].tolist()
	assert first.index(0) + 1 == first.index(1)  # (0.0, -0.0) are equal: class 0 comes right before class 1
	assert indices[1, 2].tolist() == list(range(k))  # a frame of NaNs: class order


def _autograd(z, dense, lengths, tau):
	"""float64 torch autograd of tau^2 * F.kl_div(log_softmax(z / tau), p_dense, reduction = 'sum') per utterance over its own frames."""
	zt = torch.from_numpy(np.asarray(z, dtype = np.float64)).requires_grad_(True)
	p = torch.from_numpy(dense)
	lq = F.log_softmax(zt / tau, dim = -1)
	kd = torch.stack([tau * tau * F.kl_div(lq[b, :n], p[b, :n], reduction = 'sum') for b, n in enumerate(lengths)])
	kd.sum().backward()
	return kd.detach().numpy(), zt.grad.numpy()


@pytest.mark.parametrize('C, k, tau', [(2, 1, 1.0), (38, 8, 2.0), (38, 1, 0.5), (65, 8, 0.5), (130, 32, 2.0)])
def test_kl_and_gradient_equal_float64_autograd_of_kl_div(C, k, tau):
	rng = np.random.default_rng(C + k)
	T, lengths = 13, [13, 0, 5]
	z, teacher = rng.standard_normal((3, T, C)) * 3, (rng.standard_normal((3, T, C)) * 3).astype(np.float32)
	values, indices = R.topk(teacher, k)
	kd, frames, grad = R.distill(z, values, indices, lengths, tau)
	want_kd, want_grad = _autograd(z, R.dense_teacher(values, indices, C, tau), lengths, tau)
	np.testing.assert_allclose(kd, want_kd, rtol = 1e-12, atol = 1e-12)
	np.testing.assert_allclose(grad, want_grad, rtol = 1e-12, atol = 1e-13)
	assert kd[1] == 0 and not grad[1].any() and not grad[2, 5:].any() and not frames[2, 5:].any()
	np.testing.assert_allclose(frames.sum(1), kd, rtol = 1e-12, atol = 1e-12)


@pytest.mark.parametrize('C', [8, 32])
def test_with_every_class_kept_it_is_the_full_kl(C):
	rng = np.random.default_rng(C)
	tau, T = 2.0, 6
	z, teacher = rng.standard_normal((3, T, C)) * 3, rng.standard_normal((3, T, C)) * 3
	values, indices = R.topk(teacher, C)
	kd, _, grad = R.distill(z, values, indices, [T] * 3, tau)
	p = torch.softmax(torch.from_numpy(teacher) / tau, dim = -1)  # plain softmax(z_teacher / tau): no truncation left
	want_kd, want_grad = _autograd(z, p.numpy(), [T] * 3, tau)
	np.testing.assert_allclose(kd, want_kd, rtol = 1e-12, atol = 1e-12)
	np.testing.assert_allclose(grad, want_grad, rtol = 1e-12, atol = 1e-13)
	same = R.distill(teacher, values, indices, [T] * 3, tau)
	assert np.abs(same[0]).max() < 1e-12 and np.abs(same[2]).max() < 1e-12  # a student equal to the teacher


def test_an_out_of_range_teacher_index_is_nan_in_its_frame_only():
	rng = np.random.default_rng(0)
	z = rng.standard_normal((3, 4, 5))
	values, indices = R.topk(rng.standard_normal((3, 4, 5)), 2)
	clean = R.distill(z, values, indices, [4, 4, 4], 1.0)
	indices[1, 2, 1] = 5
	kd, frames, grad = R.distill(z, values, indices, [4, 4, 4], 1.0)
	hit = np.zeros((3, 4), dtype = bool)
	hit[1, 2] = True
	assert np.array_equal(np.isnan(frames), hit) and np.array_equal(np.isnan(grad).all(-1), hit) and np.array_equal(np.isnan(grad).any(-1), hit)
	assert np.array_equal(frames[~hit], clean[1][~hit]) and np.isnan(kd[1]) and kd[0] == clean[0][0]


@pytest.mark.parametrize('C', R.CLASSES)
def test_a_float32_copy_stays_inside_the_gpu_tests_bars_on_their_inputs(C):
	worst = 0.0
	for T in R.FRAMES:
		teacher = R.distill_teacher_logits(C, T)
		for name, z in R.distill_students(C, T).items():
			for k, tau, vdt, idt in R.distill_settings(C):
				values, indices = R.topk(teacher, k)
				values = values.astype(vdt)
				assert indices.max() <= np.iinfo(idt).max
				for lengths in R.lengths_of(T):
					want = R.distill(z, values, indices.astype(idt), lengths, tau)
					got = R.distill(z, values, indices.astype(idt), lengths, tau, dtype = np.float32)
					worst = max(worst, R.check_distill(f'C {C} T {T} {name} k {k} tau {tau} {vdt} {idt} lengths {lengths}', got, want, lengths, tau, T))
	print(f'C {C}: the float32 copy uses at most {worst:.3f} of a bar')
