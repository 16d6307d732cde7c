"""uncertainty.npz: the reference's own per-frame and per-utterance uncertainty measures on one seeded batch of log-probs (3, 38, 97) --
models.entropy with sum = False, models.entropy and models.weighted_mean_entropy with lengths, models.margin (models.py:645-678), and the
entropy without the blank as vis.logits draws it: models.entropy of log_softmax over the classes [:-1] (vis.py:367-368).  float32, as torch
computes them on the CPU.  What the reference imports but is not installed is stubbed with empty modules; these functions do not reach them.

    python tests/golden/make_golden_uncertainty.py <path of the reference checkout>          (writes next to this file)
"""
import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [97, 61, 1]


class _Anything(types.ModuleType):
	"""A stand-in for a module that is not installed: any attribute is a class that can be derived from and called."""

	def __getattr__(self, name):
		if name.startswith('__'):
			raise AttributeError(name)
		return type(name, (), dict(__init__ = lambda self, *a, **k: None))


def stub(name):
	mod = _Anything(name)
	mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
	mod.__path__ = []
	sys.modules[name] = mod


def log_probs():
	g = torch.Generator().manual_seed(38)
	scale = torch.tensor([0.5, 3.0, 12.0]).view(3, 1, 1)  # flat, speech-like and saturated frames
	return torch.log_softmax(torch.randn(3, 38, 97, generator = g) * scale, dim = 1)


def import_models(root):
	sys.path.insert(0, root)
	for _ in range(32):  # stub whatever the import chain misses, one module at a time
		try:
			return importlib.import_module('models')
		except ModuleNotFoundError as e:
			stub(e.name)
			sys.modules.pop('models', None)
	raise RuntimeError('the reference models module does not import')


def main():
	if len(sys.argv) < 2 and 'CONVASR_REFERENCE' not in os.environ:
		sys.exit('usage: make_golden_uncertainty.py <path of the reference checkout>   (or CONVASR_REFERENCE)')
	models = import_models(sys.argv[1] if len(sys.argv) > 1 else os.environ['CONVASR_REFERENCE'])
	lp, lengths = log_probs(), torch.tensor(LENGTHS)
	arrays = dict(
		log_probs = lp, lengths = lengths,
		entropy_frames = models.entropy(lp, dim = 1, sum = False),
		entropy_frames_masked = models.entropy(lp, lengths, dim = 1, sum = False),
		entropy = models.entropy(lp, lengths, dim = 1),
		entropy_all_frames = models.entropy(lp, dim = 1),
		margin = torch.stack([models.margin(x, dim = 0) for x in lp]),  # (it unpacks topk's values along axis 0: one utterance (C, T) at a time, as vis.py:369 calls it)
		weighted_mean_entropy = models.weighted_mean_entropy(lp, lengths),
		entropy_no_blank = models.entropy(torch.log_softmax(lp[:, :-1], dim = 1), dim = 1, sum = False),
	)
	path = os.path.join(HERE, 'uncertainty.npz')
	np.savez_compressed(path, **{k: v.numpy() for k, v in arrays.items()})
	for k, v in arrays.items():
		print(k, tuple(v.shape), v.dtype)
	print('uncertainty.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
	main()
