"""Distillation: a teacher's top-k logits for the training step (train.train_step(..., teacher = ...)).

Online: teacher_from_model runs the big model on the batch and keeps the k largest logits of every frame (models.sparse_topk).
Offline: train.evaluate_model(..., logits_topk = k) saves them per utterance, TeacherStore packs them into one (N_frames, k) array pair
and hands a batch's rows back, padded, by one gather on the device.

A stored teacher is tied to the frames it was computed on: TeacherStore.batch raises when an utterance's stored frame count differs from
the student's output length.  That is also what happens under augment.WaveformAugment with speeds other than 1.0 (the utterance gets longer
or shorter): distil offline only without speed perturbation, or online, where the teacher sees the augmented batch.  SpecAugment keeps the
frame count and is fine."""
import torch

from . import functional as Fn
from . import models as M


def teacher_from_model(teacher_model, x, xlen, k, head = 0, values_dtype = torch.float16):
	"""(teacher, olen): the models.sparse_topk dict of teacher_model's logits[head] on the batch (x, xlen) -- k logits a frame, values in
	values_dtype, indices uint8 up to 256 classes and int16 above -- and its output lengths.  Runs under no_grad with the teacher in eval();
	its training flag and the dropout generator's offsets are restored afterwards, as train.evaluate_model does."""
	training, drop_offset = teacher_model.training, Fn._DropoutState.offset
	teacher_model.eval()
	try:
		with torch.no_grad():
			out = teacher_model(x, xlen)
			logits = out['logits'][head]
			teacher = M.sparse_topk(logits.float(), k, dim = 1, indices_dtype = torch.uint8 if logits.shape[1] <= 256 else torch.int16, values_dtype = values_dtype)
			return teacher, out['olen'][head]
	finally:
		teacher_model.train(training)
		Fn._DropoutState.offset = drop_offset


class TeacherStore:
	"""The top-k logits of a whole data set, by example id.  add() takes one utterance's (k, t) values and indices; the store keeps one
	packed (N_frames, k) array pair and the utterances' offsets.  save() / load() move data only: tensors and lists through torch.save."""

	def __init__(self):
		self.values = self.indices = None  # packed (N_frames, k)
		self.ids, self.offsets = [], [0]
		self._pending = []
		self._row = {}

	@property
	def k(self):
		self._pack()
		return 0 if self.values is None else self.values.shape[1]

	def add(self, example_id, values, indices):
		if values.ndim != 2 or values.shape != indices.shape:
			raise ValueError(f'TeacherStore.add: (k, t) values and indices expected, got {tuple(values.shape)} and {tuple(indices.shape)}')
		if int(example_id) in self._row:
			raise ValueError(f'TeacherStore.add: example {example_id} is stored already')
		self._row[int(example_id)] = len(self.ids)
		self.ids.append(int(example_id))
		self.offsets.append(self.offsets[-1] + values.shape[1])
		self._pending.append((values.t(), indices.t()))

	def add_utterances(self, meta, utterances):
		"""The per-utterance dicts of train.evaluate_model(..., logits_topk = k)['utterances']['logits'], in the order of meta."""
		for m, u in zip(meta, utterances):
			self.add(m['example_id'], u['values'], u['indices'])

	def _pack(self):
		if not self._pending:
			return
		k = self._pending[0][0].shape[1] if self.values is None else self.values.shape[1]
		if any(v.shape[1] != k for v, _ in self._pending):
			raise ValueError('TeacherStore: every utterance must hold the same k')
		dev = self._pending[0][0].device if self.values is None else self.values.device
		old = [] if self.values is None else [(self.values, self.indices)]
		self.values = torch.cat([v.to(dev) for v, _ in old + self._pending])
		self.indices = torch.cat([i.to(dev) for _, i in old + self._pending])
		self._pending = []

	def save(self, path):
		self._pack()
		torch.save(dict(values = self.values.cpu(), indices = self.indices.cpu(), ids = list(self.ids), offsets = list(self.offsets)), path)

	@classmethod
	def load(cls, path, device = None):
		d = torch.load(path, map_location = 'cpu', weights_only = True)
		store = cls()
		store.values, store.indices = d['values'].to(device), d['indices'].to(device)
		store.ids, store.offsets = [int(i) for i in d['ids']], [int(o) for o in d['offsets']]
		store._row = {e: r for r, e in enumerate(store.ids)}
		return store

	def to(self, device):
		self._pack()
		self.values, self.indices = self.values.to(device), self.indices.to(device)
		return self

	def batch(self, meta, T, olen = None):
		"""(values, indices) of logical shape (B, k, T) for the utterances of meta (their 'example_id'), padded to T frames: the rows of the
		packed arrays through one gather on the store's device.  Padding repeats the store's first row: every consumer stops at olen.
		olen: the student's output lengths, as a list or a tensor (a tensor costs one read-back).  Raises KeyError when an utterance is
		missing and ValueError when its stored frame count exceeds T or differs from olen."""
		self._pack()
		ids = [int(m['example_id'] if isinstance(m, dict) else m) for m in meta]
		missing = [e for e in ids if e not in self._row]
		if missing:
			raise KeyError(f'TeacherStore.batch: no stored teacher for example(s) {missing}')
		begin = [self.offsets[self._row[e]] for e in ids]
		count = [self.offsets[self._row[e] + 1] - b for e, b in zip(ids, begin)]
		if olen is not None:
			olen = [int(n) for n in (olen.tolist() if torch.is_tensor(olen) else olen)]
			wrong = [(e, c, n) for e, c, n in zip(ids, count, olen) if c != n]
			if wrong:
				raise ValueError(f'TeacherStore.batch: (example, stored frames, student frames) differ: {wrong} -- a stored teacher is valid only for the frames it was computed on (no speed perturbation)')
		if max(count) > T:
			raise ValueError(f'TeacherStore.batch: a stored utterance has {max(count)} frames, the batch {T}')
		dev = self.values.device
		t = torch.arange(T, device = dev).unsqueeze(0)
		begin_d, count_d = torch.tensor(begin, device = dev).unsqueeze(1), torch.tensor(count, device = dev).unsqueeze(1)
		rows = torch.where(t < count_d, begin_d + t, torch.zeros_like(t))
		return self.values[rows].permute(0, 2, 1), self.indices[rows].permute(0, 2, 1)
