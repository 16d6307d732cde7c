"""Host-side logic that needs no GPU: optimizer state in reference shapes, the fp16 / bf16 mapping of the apex opt levels, the
loss scaler's host interface, graded gradient buckets, the stride-2 fold's padding rule, the accepted configuration flags, the gradient hand-off."""
import os

import pytest
import torch

import convasr_amd as ca
from convasr_amd import functional as Fn
from convasr_amd.functional import ConvSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _small():
	torch.manual_seed(0)
	return torch.nn.Sequential(torch.nn.Conv1d(8, 16, 3), torch.nn.BatchNorm1d(16), torch.nn.Conv1d(16, 4, 1))


def test_optimizer_state_dicts_are_per_parameter_in_reference_shapes():
	"""SGD / NovoGrad state dicts (format 2): momentum as one tensor per parameter in the parameter's logical shape -- independent of the
	arena's element order -- and a round trip restores it; a flat arena-ordered buffer (the untagged pre-format-2 layout) is rejected
	with a message instead of being loaded into the wrong elements."""
	m = _small()
	flat = ca.train.FlatParameters(m)
	opt = ca.train.SGD(flat, lr = 1e-2, momentum = 0.9)
	opt.momentum_buffer.copy_(torch.arange(flat.numel, dtype = torch.float32))
	sd = opt.state_dict()
	assert sd['format'] == 2 and [tuple(t.shape) for t in sd['momentum_buffer']] == [tuple(p.shape) for p in flat.params]
	opt2 = ca.train.SGD(ca.train.FlatParameters(_small()), lr = 1e-2, momentum = 0.9)
	opt2.load_state_dict(sd)
	for a, b in zip(opt2.flat.param_views(opt2.momentum_buffer), sd['momentum_buffer']):
		assert torch.equal(a, b)
	with pytest.raises(ValueError, match = 'layout tag'):
		opt2.load_state_dict(dict(sd, momentum_buffer = torch.zeros(flat.numel)))
	with pytest.raises(ValueError, match = 'shape'):
		opt2.load_state_dict(dict(sd, momentum_buffer = [t.flatten() for t in sd['momentum_buffer']]))
	ng = ca.optimizers.NovoGrad(ca.train.FlatParameters(_small()), lr = 1e-2)
	ng.momentum_buffer.normal_()
	ng.grads_ema[0, :ng.n_seg] = torch.arange(ng.n_seg, dtype = torch.float32)
	ng.grads_ema[0, ng.n_seg] = 3.0
	nsd = ng.state_dict()
	assert nsd['steps_applied'] == 3 and nsd['grads_ema'].numel() == ng.n_seg
	ng2 = ca.optimizers.NovoGrad(ca.train.FlatParameters(_small()), lr = 1e-2)
	ng2.load_state_dict(nsd)
	assert torch.equal(ng2.grads_ema[0, :ng2.n_seg], ng.grads_ema[0, :ng.n_seg]) and float(ng2.grads_ema[0, ng2.n_seg]) == 3.0
	assert all(torch.equal(a, b) for a, b in zip(ng2.flat.param_views(ng2.momentum_buffer), ng.flat.param_views(ng.momentum_buffer)))  # (the alignment padding between parameters is not state)
	views = ng2.state
	assert all(tuple(views[p]['momentum_buffer'].shape) == tuple(p.shape) for p in ng2.flat.params)
	ng2.load_state_dict(dict(nsd, grads_ema = torch.cat([nsd['grads_ema'], torch.tensor([5.0])])))  # the earlier layout: counter behind the EMAs
	assert float(ng2.grads_ema[0, ng2.n_seg]) == 5.0


def test_opt_levels_select_fp16_like_apex_and_attach_a_loss_scaler():
	model = ca.models.JasperNet(64, [38], base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, check_time_dim_padded = False)
	flat = ca.train.FlatParameters(model)
	opt = ca.train.SGD(flat)
	assert ca.train.amp_state_dict(opt) == {}
	for level, dtype, scaler in ((None, torch.float32, False), ('O0', torch.float32, False), ('O1', torch.float16, True), ('O2', torch.float16, True), ('O3', torch.float16, False)):
		ca.models.data_parallel_and_autocast(model, opt, opt_level = level)
		assert model.compute_dtype == dtype and (flat.loss_scaler is not None) == scaler, level
	ca.models.data_parallel_and_autocast(model, opt, opt_level = 'O2', compute_dtype = torch.bfloat16)
	assert model.compute_dtype == torch.bfloat16 and flat.loss_scaler is None
	ca.models.data_parallel_and_autocast(model, opt, opt_level = 'O2', loss_scale = 128.0, keep_batchnorm_fp32 = True)
	assert flat.loss_scaler.state_dict() == dict(loss_scale = 128.0, unskipped = 0) and float(flat.loss_scaler.current[3]) == 0.0  # static: no growth window
	ca.models.data_parallel_and_autocast(model, opt, opt_level = 'O2')
	assert ca.train.amp_state_dict(opt) == dict(loss_scaler0 = dict(loss_scale = 65536.0, unskipped = 0))
	ca.train.amp_load_state_dict(opt, dict(loss_scaler0 = dict(loss_scale = 1024.0, unskipped = 17)))
	assert ca.train.amp_state_dict(opt) == dict(loss_scaler0 = dict(loss_scale = 1024.0, unskipped = 17))
	s = flat.loss_scaler
	a, b = s.pair()
	assert a.data_ptr() == s.current.data_ptr() and b.data_ptr() != a.data_ptr()
	s.advance()
	assert s.current.data_ptr() == b.data_ptr()


def test_gradient_buckets_are_graded_and_cover_the_arena():
	model = ca.models.Wav2Letter(64, [38])
	flat = ca.train.FlatParameters(model)
	engine = ca.parallel.DataParallelEngine(model, flat = flat)
	sizes = [(b['hi'] - b['lo']) * 4 / 2 ** 20 for b in engine.buckets]
	assert sizes[0] <= 4.5 and sizes[1] <= 8.5 and sizes[2] <= 16.5 and len(sizes) >= 6  # MiB: small where backward finishes last
	assert engine.buckets[0]['lo'] == 0 and all(a['hi'] <= b['lo'] for a, b in zip(engine.buckets, engine.buckets[1:]))
	assert sum(len(b['params']) for b in engine.buckets) == len(flat.params)
	assert engine.buckets[-1]['hi'] == flat.offsets[-1] + flat.params[-1].numel()


def test_fold2_pads_only_when_the_conv_output_is_unchanged():
	"""The zero frame in front of the stride-2 prologue (functional.Fold2.wants_even_input): only for an odd frame count, an odd kernel
	(the output length must not change) and channel counts inside the fold's envelope."""
	want = Fn.Fold2.wants_even_input
	assert want((256, 64, 11), ConvSpec(11, 2, 1, 5), 1501)
	assert not want((256, 64, 11), ConvSpec(11, 2, 1, 5), 1502)   # already even
	assert not want((256, 64, 12), ConvSpec(12, 2, 1, 6), 1501)   # even kernel: one more output frame with the padded input
	assert not want((256, 40, 11), ConvSpec(11, 2, 1, 5), 1501)   # 2 * Cin not a multiple of 128
	assert not want((200, 64, 11), ConvSpec(11, 2, 1, 5), 1501)   # Cout not a multiple of 128
	assert not want((256, 64, 11), ConvSpec(11, 1, 1, 5), 1501)   # not strided


def test_accepted_configuration_flags_build_the_reference_state_dict_layout():
	kw = dict(base_width = 32, kernel_sizes = [11, 13], out_width_factors = [2, 2], dropouts = [0.2, 0.2], out_width_factors_large = [2, 2], repeat = 2, num_subblocks = 1)
	plain = ca.models.JasperNet(64, [38], **kw)
	assert list(ca.models.JasperNet(64, [38], inplace = True, **kw).state_dict()) == list(plain.state_dict())
	sep = ca.models.JasperNet(64, [38], separable = True, groups = 16, **kw)
	keys = list(sep.state_dict())
	assert 'backbone.1.conv.0.0.bias' in keys and 'backbone.1.conv.0.2.weight' in keys and tuple(sep.state_dict()['backbone.1.conv.0.0.weight'].shape) == (64, 4, 11)
	assert 'backbone.0.conv.0.0.bias' not in keys  # the prologue is not separable (models.py:200-211)
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window', stft_mode = 'conv')
	assert tuple(fe.state_dict()['stft.weight'].shape) == (514, 1, 512)
	with pytest.raises(ValueError):
		ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window', stft_mode = 'fft2')
	norm = ca.models.MaskedInstanceNorm1d(64, affine = False, track_running_stats = False, legacy = False)
	assert norm.legacy is False
	bpe = ca.models.JasperNet(64, [38, 48], decoder_type = 'bpe', **kw)
	assert any(k.startswith('decoder.1.1.bn.0') for k in bpe.state_dict())
	for name in ('JasperNetSeparable', 'JasperNetBigInplace', 'Wav2LetterDenseNoDilationInplace', 'JasperNetLarge', 'Wav2Letter'):
		assert hasattr(ca.models, name)


def test_ctc_workspace_query_follows_the_state_split():
	"""convasr_ctc_workspace_bytes is host code (no GPU call): lattice rows hold 128 (NPH + NPL) states, the smallest split that covers
	the 2 S + 1 states of the extended target -- (1,1) up to 127 labels, (2,1) to 191, ... (4,4) to 511, (5,4) ... (8,8) to 1,023; longer targets are refused (-1)."""
	from convasr_amd import _lib
	lib = _lib.load()
	B, T = 3, 753
	NB = T // 8 + 1
	for S, cap in [(0, 256), (1, 256), (127, 256), (128, 384), (150, 384), (191, 384), (192, 512), (255, 512), (256, 640), (319, 640), (320, 768), (383, 768), (384, 896), (447, 896), (448, 1024), (511, 1024), (512, 1152), (575, 1152), (576, 1280), (831, 1664), (832, 1792), (959, 1920), (960, 2048), (1023, 2048)]:
		want = (2 * B * T * cap + 4 * B * NB + 2 * B) * 4
		assert lib.convasr_ctc_workspace_bytes(B, T, S) == want, (S, cap)
	assert lib.convasr_ctc_workspace_bytes(B, T, 1024) == -1


def test_every_named_configuration_of_the_reference_builds_the_same_network():
	"""`getattr(models, args.model)` (train.py:428, transcribe.py:44): all 24 JasperNet subclasses of the reference's models.py (819-1442) exist
	here under the same names and build the same network -- per block the conv / batch-norm / residual-branch geometry, activation, dropout and
	mask flag, the residual policy, the feature normalisation's flags, every state-dict key and shape -- as the reference's own constructors did
	(tests/golden/model_zoo.json, written by make_golden_r5.py through tests/golden/describe_model.py)."""
	import json
	import sys
	import convasr_amd as ca
	sys.path.insert(0, GOLDEN)
	from describe_model import describe
	zoo = json.load(open(os.path.join(GOLDEN, 'model_zoo.json')))
	assert len(zoo) == 27
	for key, want in sorted(zoo.items()):
		name, _, variant = key.partition(':')
		cls = getattr(ca.models, name)
		kw = dict(base_width = 128 if 'Separable' in name else 16)
		args = (64, [38, 300]) if variant == 'bpe' else (64, [38])
		if variant == 'bpe':
			kw['decoder_type'] = 'bpe'
		got = json.loads(json.dumps(describe(cls(*args, **kw))))
		for field in want:
			assert got[field] == want[field], (key, field)


def test_split_network_wiring_decides_which_outputs_exist_as_planes_only():
	"""Round 6, host logic only: in a split-operand network (set_compute_dtype('bf16x3')) a layer output is handed on as its 16-bit planes ONLY when
	its one reader is a split conv -- the next repeat of the block, or the first conv of the block the network wired behind it (feeds_block);
	the last block (its reader is the decoder), tapped outputs of residual networks, evaluation mode and plain fp32 keep real fp32 outputs."""
	import torch
	import convasr_amd as ca
	flags = lambda m: [[blk._planes_out(r, r == len(blk.conv) - 1) for r in range(len(blk.conv))] for blk in m.backbone]
	m = ca.models.Wav2Letter(64, [38], compute_dtype = 'bf16x3').train()
	assert m.compute_dtype == torch.float32 and m.split_dtype == torch.bfloat16 and m.decoder.split_dtype == torch.bfloat16
	f = flags(m)
	assert all(all(row) for row in f[:-1]) and f[-1] == [False], f  # 17 of the 18 layer outputs exist as planes only; the last feeds the head
	assert [blk.feeds_block is not None for blk in m.backbone] == [True] * 7 + [False]
	m.eval()
	assert not any(any(row) for row in flags(m))
	m.train()
	m.set_compute_dtype(torch.float32)
	assert m.split_dtype is None and not any(any(row) for row in flags(m))
	m.set_compute_dtype('f16x3', inference = True)
	assert m.split_dtype == torch.float16 and all(blk.split_inference for blk in m.backbone) and all(all(row) for row in flags(m)[:-1])
	# a dense-residual network: block outputs that later blocks tap have several readers -> real tensors; repeats inside a block still hand planes on
	j = ca.models.JasperNet(64, [38], base_width = 64, kernel_sizes = [11, 13], out_width_factors = [2, 3], dropouts = [0.0, 0.0], out_width_factors_large = [4, 4], residual = 'dense', repeat = 2, compute_dtype = 'bf16x3').train()
	fj = flags(j)
	tapped = [blk.tapped_output for blk in j.backbone]
	for blk, row, tap in zip(j.backbone, fj, tapped):
		assert row[:-1] == [True] * (len(row) - 1)  # inside a block: the next repeat is the one reader
		assert row[-1] == (not tap and blk.feeds_block is not None), (row, tap)
	assert any(tapped) and not fj[-1][-1]
	# state-dict keys are untouched by the wiring (feeds_block is a weak reference, not a registered submodule)
	assert not any('feeds_block' in k for k in j.state_dict())


def test_split_operand_arithmetic_restated_on_the_cpu():
	"""What the MI355X split-operand path claims, checked on the CPU against float64 (oracle.conv1d_split3, the restatement of its arithmetic): two
	bf16 planes hold 16 significant bits (fp16: 22, above its subnormal range), x - hi is exact, and a conv formed from the three kept
	products sits 2^-17 .. 2^-16 from the float64 conv -- three orders of magnitude inside plain bf16's 2^-9 -- with the dropped lo x lo
	term accounting for what is left."""
	import torch
	import torch.nn.functional as F
	from oracle import convasr_oracle as O
	torch.manual_seed(0)
	x = torch.randn(3, 64, 200) * torch.logspace(-2, 1, 64).view(1, 64, 1)
	w = torch.randn(96, 64, 11) / (64 * 11) ** 0.5
	for dt, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
		hi, lo = O.split_planes(x, dt)
		assert torch.equal((x - hi).to(dt).float(), lo) and bool(((hi + lo - x).abs() <= x.abs() * 2.0 ** (-2 * bits) + (2.0 ** -25 if dt == torch.float16 else 0)).all())
	ref = F.conv1d(x.double(), w.double(), padding = 5)
	rel = lambda a: float((a.double() - ref).norm() / ref.norm())
	e3 = rel(O.conv1d_split3(x, w, padding = 5))
	e1 = rel(F.conv1d(x.bfloat16().double(), w.bfloat16().double(), padding = 5))
	assert 1e-6 < e3 < 8e-6 and e1 > 300 * e3, (e3, e1)  # measured on the MI355X kernels: 4.5e-6 and 2.3e-3
	xh, xl = O.split_planes(x); wh, wl = O.split_planes(w)
	full = O.conv1d_split3(x, w, padding = 5) + F.conv1d(xl.double(), wl.double(), padding = 5)  # + the dropped term: what is left is the planes' own residue
	assert rel(full) < 0.8 * e3
	assert rel(O.conv1d_split3(x, w, padding = 5, dtype = torch.float16)) < 5e-7


# ------------------------------------------------------------------------------------------------ the gradient hand-off (functional._deliver_many)

def _arena_param(shape, fresh = True, fired = None):
	"""A CPU parameter carrying what train.FlatParameters / the data-parallel engine hang on it: a gradient arena, the fresh flag, a ready hook."""
	p = torch.nn.Parameter(torch.zeros(shape))
	p._convasr_grad, p._convasr_fresh = torch.zeros(shape), fresh
	if fired is not None:
		p._convasr_ready = lambda q: fired.append(q)
	return p


@pytest.mark.parametrize('fresh', [True, False])
def test_hand_off_writes_arena_groups_in_place_and_fires_the_hooks_after_compute(fresh):
	"""Every live parameter of the group has an arena: compute gets the arenas and accumulate = not fresh, autograd gets None, the parameters
	stop being fresh, and each live parameter's ready hook fires once -- after compute.  A parameter that needs no gradient gets None."""
	fired, log = [], []
	w, b, frozen = _arena_param((4, 3), fresh, fired), _arena_param((4, ), fresh, fired), _arena_param((2, ), fresh, fired)
	frozen.requires_grad_(False)

	def compute(outs, acc):
		log.append((outs, acc, list(fired)))
	ret = Fn._deliver([w, None, b, frozen], compute)
	assert ret == [None, None, None, None]
	(outs, acc, fired_before), = log
	assert outs[0] is w._convasr_grad and outs[1] is None and outs[2] is b._convasr_grad and outs[3] is None
	assert acc is (not fresh) and fired_before == []
	assert w._convasr_fresh is False and b._convasr_fresh is False and frozen._convasr_fresh is fresh
	assert len(fired) == 2 and fired[0] is w and fired[1] is b


def test_hand_off_refuses_a_group_out_of_step_before_compute_runs():
	ran = []
	w, b = _arena_param((4, 3), True), _arena_param((4, ), False)
	with pytest.raises(ca._lib.ConvasrHipError, match = 'gradient arenas of one layer are out of step'):
		Fn._deliver([w, b], lambda outs, acc: ran.append(1))
	with pytest.raises(ca._lib.ConvasrHipError, match = 'gradient arenas of one layer are out of step'):
		Fn._deliver_many([[_arena_param((2, ))], [w, b]], lambda outs, accs: ran.append(1))
	assert not ran and w._convasr_fresh is True and b._convasr_fresh is False


def test_hand_off_returns_fresh_fp32_tensors_for_a_group_without_arenas():
	"""One live parameter without an arena is enough: the whole group goes to autograd as fresh fp32 contiguous tensors, never accumulated."""
	fired = []
	w, b = torch.nn.Parameter(torch.zeros(4, 3, 2, dtype = torch.float64).permute(0, 2, 1)), _arena_param((4, ), False, fired)
	seen = []
	ret = Fn._deliver([w, b, None], lambda outs, acc: seen.append((outs, acc)))
	(outs, acc), = seen
	assert acc is False and ret[2] is None and outs[2] is None
	for r, o, p in zip(ret[:2], outs[:2], (w, b)):
		assert r is o and r.dtype == torch.float32 and r.is_contiguous() and r.shape == p.shape and r is not getattr(p, '_convasr_grad', None)
	assert b._convasr_fresh is False and not fired  # (nothing was delivered into the arena)


def test_hand_off_of_several_groups_runs_compute_once():
	"""Arena groups (one fresh, one accumulating), a group for autograd and a group nobody wants, in one call: one compute with per-group
	outputs and flags; hooks only for the arena groups, after it."""
	fired, log = [], []
	a, b, c = [_arena_param((3, ), True, fired), _arena_param((3, ), True, fired)], [_arena_param((3, ), False, fired), None], [torch.nn.Parameter(torch.zeros(3)), None]
	dead = [_arena_param((3, ), True, fired).requires_grad_(False), None]
	ret = Fn._deliver_many([a, b, c, dead], lambda outs, accs: log.append((outs, accs, len(fired))))
	(outs, accs, fired_before), = log
	assert accs == [False, True, False, False] and fired_before == 0
	assert outs[0][0] is a[0]._convasr_grad and outs[0][1] is a[1]._convasr_grad and outs[1][0] is b[0]._convasr_grad and outs[1][1] is None and outs[3] == [None, None]
	assert ret[0] == [None, None] and ret[1] == [None, None] and ret[2][0] is outs[2][0] and ret[2][1] is None and ret[3] == [None, None]
	assert [id(p) for p in fired] == [id(a[0]), id(a[1]), id(b[0])]


def test_hand_off_with_no_live_parameter_runs_compute_only_when_told_to():
	"""Nothing wants a gradient: compute is skipped -- unless it produces more than gradients (the batch-norm backward's coefficients:
	always = True), then it runs once with all-None outputs."""
	gamma, beta = _arena_param((4, )).requires_grad_(False), _arena_param((4, )).requires_grad_(False)
	log = []
	assert Fn._deliver([gamma, beta], lambda outs, acc: log.append((outs, acc))) == [None, None] and not log
	assert Fn._deliver_many([[gamma, beta], [None, None]], lambda outs, accs: log.append((outs, accs))) == [[None, None], [None, None]] and not log
	assert Fn._deliver([gamma, None], lambda outs, acc: log.append((outs, acc)), always = True) == [None, None]
	assert Fn._deliver_many([[gamma, beta], [None]], lambda outs, accs: log.append((outs, accs)), always = True) == [[None, None], [None]]
	assert log == [([None, None], False), ([[None, None], [None]], [False, False])]
	assert gamma._convasr_fresh is True


def test_a_repeated_library_query_is_answered_from_memory(monkeypatch):
	"""ops._cached_query: the row count of the conv statistics and the weight gradient's workspace size are pure functions of their integer
	arguments and sit on every launch's path -- the second identical question must not reach the library (nor any other helper of that name)."""
	from convasr_amd import ops, _lib
	rows = ops._conv_stats_max_rows(3, 777)
	geometry = (3, 128, 256, 777, 777, 5, 1, 2)
	nbytes = ops._cached_query('convasr_conv1d_wgrad_workspace_bytes', *geometry)
	assert rows > 0 and nbytes >= 0 and ops._queries[('convasr_conv_stats_max_rows', 3, 777)] == rows and ops._queries[('convasr_conv1d_wgrad_workspace_bytes', ) + geometry] == nbytes

	def unreachable():
		raise AssertionError('a memoised query reached the library again')
	monkeypatch.setattr(_lib, 'load', unreachable)
	assert ops._conv_stats_max_rows(3, 777) == rows and ops._cached_query('convasr_conv1d_wgrad_workspace_bytes', *geometry) == nbytes
	with pytest.raises(AssertionError, match = 'reached the library'):
		ops._conv_stats_max_rows(3, 778)


def test_a_refused_library_query_raises_with_its_message_and_is_not_remembered():
	"""ops._query: a negative answer raises with the library's message and is never stored -- the same question asked again reaches the
	library again and reports its own message, not whatever another refusal left in convasr_last_error() meanwhile."""
	import re
	from convasr_amd import ops, _lib
	lib = _lib.load()
	name, args = 'convasr_ctc_loss_long_workspace_bytes', (2, 500, 38, 131072)
	assert lib.convasr_ctc_loss_long_workspace_bytes(*args) < 0
	message = lib.convasr_last_error().decode()
	assert '131072' in message
	for _ in range(2):
		assert lib.convasr_nw_align_workspace_bytes(0, 5, 5) < 0 and lib.convasr_last_error().decode() != message  # another refusal in between
		with pytest.raises(_lib.ConvasrHipError, match = re.escape(f'{name} failed: {message}')):
			ops._query(name, *args)
		assert (name, ) + args not in ops._queries
	good = (2, 500, 38, 1024)
	assert ops._query(name, *good) == lib.convasr_ctc_loss_long_workspace_bytes(*good) == ops._queries[(name, ) + good] > 0


def test_frame_lengths_of_the_decoding_wrappers():
	from convasr_amd import ops
	cpu = torch.device('cpu')
	full = ops._frame_lengths('f', None, 3, 7, cpu)
	assert full.dtype == torch.int64 and full.tolist() == [7, 7, 7] and full.device == cpu
	for given in ([5, 0, 7], torch.tensor([5, 0, 7], dtype = torch.int32), torch.tensor([[5, 1], [0, 1], [7, 1]], dtype = torch.int32)[:, 0]):
		got = ops._frame_lengths('f', given, 3, 7, cpu)
		assert got.dtype == torch.int64 and got.is_contiguous() and got.tolist() == [5, 0, 7]
	for bad in ([5, 7], [[5, 0, 7]], 5):
		with pytest.raises(ValueError, match = 'ctc_greedy_collapse: lengths of shape .* for a batch of 3'):
			ops._frame_lengths('ctc_greedy_collapse', bad, 3, 7, cpu)


def test_ctc_targets_of_the_loss_and_alignment_wrappers():
	from convasr_amd import ops
	cpu = torch.device('cpu')
	B, S = 3, 4
	flat = torch.arange(B * S, dtype = torch.int32)
	lens = torch.tensor([[4, 9], [2, 9], [0, 9]], dtype = torch.int32)
	targets, il, tl = ops._ctc_targets(flat, torch.tensor([10, 9, 8], dtype = torch.int32), lens[:, 0], B, cpu)
	assert targets.shape == (B, S) and targets.tolist() == flat.view(B, S).tolist()
	assert all(t.dtype == torch.int64 and t.is_contiguous() and t.device == cpu for t in (targets, il, tl))
	assert il.tolist() == [10, 9, 8] and tl.tolist() == [4, 2, 0] and not lens[:, 0].is_contiguous()
	wide = torch.arange(B * 2 * S).view(B, 2 * S)[:, ::2]  # a strided (B, S) view
	targets, _, _ = ops._ctc_targets(wide, il, tl, B, cpu)
	assert targets.shape == (B, S) and targets.is_contiguous() and torch.equal(targets, wide)
