"""The host side of distillation, without a GPU: models.sparse_topk / sparse_topk_todense on CPU tensors, distill.TeacherStore, the wiring
of the two new entry points (header, _lib, exported symbols) and their envelope, which is checked before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('convasr_topk_frames_max_k', 'convasr_topk_frames', 'convasr_distill_kl')
_DUMMY = (ctypes.c_char * 64)()


@pytest.mark.parametrize('dim, largest', [(1, True), (-2, True), (-1, True), (1, False)])
@pytest.mark.parametrize('indices_dtype, values_dtype', [(None, None), (torch.int16, torch.float16), (torch.uint8, torch.float32), (torch.int32, None)])
def test_sparse_topk_on_cpu_tensors_is_torch_topk_and_a_scatter(dim, largest, indices_dtype, values_dtype):
	from convasr_amd import models
	x = torch.randn(2, 9, 7, generator = torch.Generator().manual_seed(3))
	saved = models.sparse_topk(x, 3, dim = dim, largest = largest, indices_dtype = indices_dtype, values_dtype = values_dtype, fill_value = -1.5)
	want = torch.topk(x, 3, dim = dim, largest = largest)
	assert sorted(saved) == sorted(['k', 'dim', 'largest', 'shape', 'dtype', 'device', 'fill_value', 'indices', 'values'])
	assert (saved['k'], saved['dim'], saved['largest'], saved['shape'], saved['dtype'], saved['device'], saved['fill_value']) == (3, dim, largest, x.shape, torch.float32, x.device, -1.5)
	assert saved['indices'].dtype == (indices_dtype or torch.int64) and saved['values'].dtype == (values_dtype or torch.float32)
	assert torch.equal(saved['indices'].long(), want.indices) and torch.equal(saved['values'], want.values.to(values_dtype or torch.float32))
	dense = models.sparse_topk_todense(saved)
	kept = want.values.to(values_dtype or torch.float32).float()
	assert dense.dtype == x.dtype and torch.equal(dense, torch.full_like(x, -1.5).scatter_(dim, want.indices, kept))
	assert torch.equal(models.sparse_topk_todense(saved, device = 'cpu'), dense)


def _utterance(rng, k, t, C = 38):
	x = torch.from_numpy(rng.standard_normal((C, t)).astype(np.float32))
	top = torch.topk(x, k, dim = 0)
	return top.values.half(), top.indices.to(torch.uint8)


def test_teacher_store_round_trip_and_refusals(tmp_path):
	from convasr_amd.distill import TeacherStore
	rng = np.random.default_rng(5)
	utts = {11: _utterance(rng, 4, 9), 7: _utterance(rng, 4, 1), 23: _utterance(rng, 4, 14)}
	store = TeacherStore()
	for e, (v, i) in utts.items():
		store.add(e, v, i)
	with pytest.raises(ValueError):
		store.add(7, *utts[7])  # stored already
	with pytest.raises(ValueError):
		store.add(8, utts[7][0], utts[11][1])  # shapes differ
	path = str(tmp_path / 'teacher.pt')
	store.save(path)
	saved = torch.load(path, weights_only = True)  # data only: tensors and lists
	assert sorted(saved) == ['ids', 'indices', 'offsets', 'values'] and saved['values'].shape == (24, 4) and saved['offsets'] == [0, 9, 10, 24] and saved['ids'] == [11, 7, 23]
	for s in (store, TeacherStore.load(path, 'cpu')):
		assert s.k == 4
		meta = [dict(example_id = 23), dict(example_id = 7)]
		values, indices = s.batch(meta, 16, olen = [14, 1])
		assert values.shape == (2, 4, 16) and indices.shape == (2, 4, 16) and values.dtype == torch.float16 and indices.dtype == torch.uint8
		assert values.stride() == (64, 1, 4)  # (B, T, k) memory, as ops.topk_frames hands it out
		assert torch.equal(values[0, :, :14], utts[23][0]) and torch.equal(indices[0, :, :14], utts[23][1])
		assert torch.equal(values[1, :, :1], utts[7][0]) and torch.equal(indices[1, :, :1], utts[7][1])
		assert torch.equal(s.batch(meta, 16, olen = torch.tensor([14, 1]))[0], values) and torch.equal(s.batch([23, 7], 16)[1], indices)
		with pytest.raises(KeyError):
			s.batch([dict(example_id = 5)], 16)
		with pytest.raises(ValueError):
			s.batch(meta, 16, olen = [13, 1])  # the student has other frames than the teacher had: e.g. a speed-perturbed utterance
		with pytest.raises(ValueError):
			s.batch(meta, 8)


def test_wiring_and_the_envelope_checked_before_any_launch():
	from convasr_amd import _lib
	header = open(os.path.join(ROOT, 'include', 'convasr_hip.h')).read()
	lib = _lib.load()
	for name in NEW:
		assert re.search(r'\b' + name + r'\s*\(', header), name
		assert name in _lib._SIGNATURES and hasattr(lib, name), name
	assert 'CONVASR_ABI_VERSION 11' in header and lib.convasr_abi_version() == 11
	assert '#define CONVASR_TOPK_MAX_K 32' in header and lib.convasr_topk_frames_max_k() == 32 == _lib.TOPK_MAX_K
	for name, code in (('U8', _lib.INDEX_U8), ('I16', _lib.INDEX_I16), ('I32', _lib.INDEX_I32)):
		assert f'#define CONVASR_INDEX_{name} {code}' in header
	# no GPU is touched: every refusal precedes the first HIP call
	one = ctypes.cast(_DUMMY, ctypes.c_void_p)
	f32, f16, einval = _lib.F32, _lib.F16, -1
	base = dict(vdt = f32, idt = _lib.INDEX_I32, B = 1, T = 8, C = 38, k = 5, tau = 1.0)
	bad = [dict(k = 0), dict(k = 33, C = 64), dict(k = 3, C = 2), dict(idt = _lib.INDEX_U8, C = 257), dict(C = 1, k = 1), dict(C = 8193), dict(B = 0), dict(T = 0), dict(B = 1 << 16, T = 1 << 15),
	       dict(vdt = _lib.BF16), dict(idt = 3)]
	for kw in bad:
		a = dict(base, **kw)
		assert lib.convasr_topk_frames(one, one, a['vdt'], one, a['idt'], a['B'], a['T'], a['C'], a['k'], None) == einval, kw
		assert b'topk_frames' in lib.convasr_last_error()
	for kw in bad + [dict(tau = 0.0), dict(tau = -1.0), dict(tau = float('inf')), dict(tau = float('nan'))]:
		a = dict(base, **kw)
		assert lib.convasr_distill_kl(one, one, a['vdt'], one, a['idt'], one, one, one, one, a['B'], a['T'], a['C'], a['k'], a['tau'], None) == einval, kw
		assert b'distill_kl' in lib.convasr_last_error()
	assert lib.convasr_topk_frames(None, one, f32, one, _lib.INDEX_I32, 1, 8, 38, 5, None) == einval
	assert lib.convasr_distill_kl(one, one, f16, one, _lib.INDEX_U8, None, one, one, None, 1, 8, 38, 5, 1.0, None) == einval  # no lengths
	assert lib.convasr_distill_kl(one, one, f16, one, _lib.INDEX_U8, one, one, None, None, 1, 8, 38, 5, 1.0, None) == einval  # no kd_frames


def test_teacher_of_the_wrong_kind_is_refused():
	from convasr_amd import functional as Fn
	x = torch.randn(2, 5, 7)
	top = torch.topk(x, 2, dim = 2)
	with pytest.raises(ValueError):
		Fn._teacher_pair(dict(k = 2, dim = -1, largest = True, shape = x.shape, values = top.values, indices = top.indices))
	with pytest.raises(ValueError):
		Fn._teacher_pair(dict(k = 2, dim = 1, largest = False, shape = x.shape, values = top.values, indices = top.indices))
