"""Per-launch times of the two things the epilogue work after round 6 touches, for an A/B of two builds (run once per library with
CONVASR_HIP_LIB=..., alternating; the parent build ignores debug bit 16):
  * the dgrad launches with the fused BN-backward epilogue on stored gates (conv_v2s.hip, BNF = 2) next to the plain launch of the same conv;
  * the forward launches whose last partial round fills at most a quarter of the CUs, with quarter tiles and with half tiles (debug bit 16).
Same-process interleaved timing, best of three rounds of 20 launches; prints one JSON line.  AB_DTYPE=f16: fp16 instead of bf16."""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from convasr_amd import ops, _lib
d = torch.device('cuda:0'); dt = torch.float16 if os.environ.get('AB_DTYPE') == 'f16' else torch.bfloat16; torch.manual_seed(0)
lib = _lib.load()
B, T = 64, 751
ACT = (_lib.ACT_HARDTANH, 0.0, 20.0)
def timeit(fn, n = 20):
	for _ in range(3): fn()
	e0, e1 = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
	torch.cuda.synchronize(); e0.record()
	for _ in range(n): fn()
	e1.record(); torch.cuda.synchronize()
	return e0.elapsed_time(e1) / n * 1e3
out = dict(lib = os.path.basename(_lib.LIB_PATH), dtype = str(dt), fused = {}, narrow = {})
# (dx channels, dy channels, K, dil) of dgrad launches of the Wav2Letter step
for (c, cdy, k, dil) in [(256, 256, 11, 1), (384, 384, 11, 1), (384, 512, 11, 1), (768, 768, 11, 1), (768, 896, 29, 2)]:
	pad = dil * (k - 1) - dil * (k // 2)
	dy = ops.as_cl(torch.randn(B, cdy, T, device = d), dt)
	w = torch.randn(cdy, c, k, device = d) / (cdy * k) ** 0.5
	_, dgr = ops.pack_weight(w, dt, None)
	yb = ops.as_cl(torch.randn(B, c, T, device = d) * 4 + 2, dt)
	sc, sh, mean, istd = (torch.rand(c, device = d) + 0.5 for _ in range(4))
	xl = torch.ones(B, device = d)
	gate = torch.zeros(B * T * c // 8, dtype = torch.uint8, device = d)
	ops.bn_act(yb, sc, sh, ACT, xlen = xl, dropout_p = 0.2, seed = 1, offset = 0, gate = gate)
	sums = ops.ConvStats(c, B, T, d)
	plain = lambda: ops.conv1d(dy, dgr, c, k, 1, dil, pad)
	fused = lambda: ops.conv1d_dgrad_bn_reduce(dy, dgr, c, k, dil, pad, yb, sc, sh, mean, istd, ACT, 0.2, 1, 0, xl, sums, gate = gate)
	assert torch.equal(plain(), fused())
	tp, tf = [], []
	for _ in range(3):
		tp.append(timeit(plain)); tf.append(timeit(fused))
	out['fused'][f'{cdy}->{c} k{k} d{dil}'] = dict(plain_us = round(min(tp), 1), fused_us = round(min(tf), 1), extra_us = round(min(tf) - min(tp), 1))
	del dy, w, dgr, yb, gate
for (cin, cout, k, dil) in [(768, 896, 29, 2), (256, 384, 11, 1), (384, 384, 11, 1), (512, 384, 11, 1)]:
	x = ops.as_cl(torch.randn(B, cin, T, device = d).clamp_(0, 20), dt)
	w = torch.randn(cout, cin, k, device = d) / (cin * k) ** 0.5
	wp = ops.pack_weight(w, dt, _lib.PACK_FWD)
	stats = ops.ConvStats(cout, B, T, d)
	run = lambda: ops.conv1d(x, wp, cout, k, 1, dil, dil * (k // 2), stats = stats)
	res, ref = {}, None
	for _ in range(3):
		for name, bits in (('quarters', 0), ('halves', 16), ('full', 32)):
			lib.convasr_debug_set_conv_v2(1 | (bits << 8))
			y = run()
			ref = y.clone() if ref is None else ref
			assert torch.equal(ref, y), (cin, cout, name)
			res.setdefault(name, []).append(timeit(run))
	lib.convasr_debug_set_conv_v2(1)
	out['narrow'][f'{cin}->{cout} k{k} d{dil}'] = {n: round(min(v), 1) for n, v in res.items()}
	del x, w, wp
print(json.dumps(out), flush = True)
