"""Hot phrases for the CTC beam search (include/convasr_hip.h: convasr_ctc_beam_search_hot; contextual biasing, as pyctcdecode's
hotwords or a context graph do it).

HotWords(phrases, labels) turns a list of phrases into the flat trie the kernel walks.  A phrase is lowercased and stripped, runs of
inner whitespace become one space, duplicates are merged; every character must be a label, and the labels need exactly one space.
Device tables (uploaded once per device by HotWords.device_tables), laid out as lm.NgramLM lays out its vocabulary trie:
  hot_mask  (n_nodes, MW) uint32, MW = ceil(C / 32): bit c set when the node has a child by class c (node 0 is the root)
  hot_child (n_nodes,) int32: the node id of the node's first child; the child by class c is hot_child + (number of set bits below c)
  hot_term  (n_nodes,) int32: 1 when a phrase ends at the node, else 0
The rule (normative in the header): a prefix carries a trie node u (or DEAD) and the number k of labels matched since the last completed
phrase.  Appending c to it adds +w when u has a child by c; otherwise the pending k labels give their bonus back, -(w * k), and a new match
starts (+w) when the prefix ends in the space and the root has a child by c.  At the end of the utterance a pending match gives its bonus
back too.  So a phrase that was completed keeps w per label, everything else nets zero.  No weight has been tuned on speech here."""
import numpy as np

from . import lm as lm_mod

DEAD = -1


def normalize(phrase):
	return ' '.join(str(phrase).lower().split())


class HotWords:
	"""phrases: an iterable of strings; labels: one character per class (lowercased, as lm.parse_labels reads them)."""

	def __init__(self, phrases, labels):
		self.labels = lm_mod.parse_labels(labels)
		self.num_classes = len(self.labels)
		if self.labels.count(' ') != 1:
			raise ValueError(f'HotWords: the labels need exactly one space class, got {self.labels.count(" ")}')
		self.space = self.labels.index(' ')
		cls = {}
		for c, ch in enumerate(self.labels):
			cls.setdefault(ch, c)
		self.char_class = cls
		if isinstance(phrases, str):
			raise TypeError('HotWords: phrases must be a list of strings, not one string')
		self.phrases, self.encoded = [], []
		seen = set()
		for raw in phrases:
			p = normalize(raw)
			if not p:
				raise ValueError(f'HotWords: empty phrase {raw!r}')
			bad = sorted({ch for ch in p if ch not in cls})
			if bad:
				raise ValueError(f'HotWords: the phrase {p!r} has characters that are no label: {"".join(bad)!r}')
			if p not in seen:
				seen.add(p)
				self.phrases.append(p)
				self.encoded.append(tuple(cls[ch] for ch in p))
		self._cache = {}
		self._build()

	def _build(self):
		children, term = [{}], [0]
		for cs in self.encoded:
			nd = 0
			for c in cs:
				nx = children[nd].get(c)
				if nx is None:
					nx = children[nd][c] = len(children)
					children.append({}); term.append(0)
				nd = nx
			term[nd] = 1
		# breadth-first, children sorted by class: the nodes of one parent are contiguous (lm.NgramLM.tables)
		n, MW = len(children), (self.num_classes + 31) // 32
		order, remap, head = [0], {0: 0}, 0
		first_child = np.zeros(n, dtype = np.int32)
		while head < len(order):
			old = order[head]
			first_child[head] = len(order)
			for c in sorted(children[old]):
				remap[children[old][c]] = len(order)
				order.append(children[old][c])
			head += 1
		mask = np.zeros((n, MW), dtype = np.uint32)
		terminal = np.zeros(n, dtype = np.int32)
		self._children = [None] * n
		for new, old in enumerate(order):
			terminal[new] = term[old]
			self._children[new] = {c: remap[k] for c, k in children[old].items()}
			for c in children[old]:
				mask[new, c >> 5] |= np.uint32(1 << (c & 31))
		self._tables = (mask, first_child, terminal)

	@property
	def num_nodes(self):
		return int(self._tables[2].shape[0])

	def words(self):
		"""The words of the phrases (split at the space), in order of first appearance."""
		out = []
		for p in self.phrases:
			for w in p.split(' '):
				if w not in out:
					out.append(w)
		return out

	def tables(self, blank):
		"""(hot_mask, hot_child, hot_term) for a given blank class: the same trie for every blank, but no phrase may hold its character."""
		blank = int(blank)
		if not 0 <= blank < self.num_classes:
			raise ValueError(f'HotWords: blank {blank} outside [0, {self.num_classes})')
		if blank == self.space:
			raise ValueError(f'HotWords: the space class {self.space} is the blank')
		for p, cs in zip(self.phrases, self.encoded):
			if blank in cs:
				raise ValueError(f'HotWords: the phrase {p!r} holds the character of the blank, {self.labels[blank]!r}')
		return self._tables

	def device_tables(self, blank, device):
		"""The tables as device tensors (uploaded once per device and blank)."""
		import torch
		key = (int(blank), str(device))
		if key not in self._cache:
			mask, child, term = self.tables(blank)
			t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
			self._cache[key] = dict(hot_mask = t(mask.view(np.int32)), hot_child = t(child), hot_term = t(term))
		return self._cache[key]

	def check_vocabulary(self, lm, blank):
		"""With an LM every word of every phrase must be a word of its vocabulary V: ValueError naming the others."""
		key = ('vocabulary', id(lm), int(blank))
		if key not in self._cache:
			V = lm.vocabulary_of(int(blank))
			self._cache[key] = [w for w in self.words() if w not in V]
		missing = self._cache[key]
		if missing:
			raise ValueError(f'HotWords: not in the language model\'s vocabulary for these labels: {", ".join(repr(w) for w in missing)} '
			                 '(hot words outside the vocabulary are not supported with an LM)')

	def bonus(self, tokens, weight = 1.0):
		"""The hot score a labelling (a list of classes without blanks) collects at `weight`: the sum of the deltas of its extensions plus the
		end-of-utterance term -(weight * pending)."""
		w = float(weight)
		u, k, last, total = 0, 0, -1, 0.0
		for c in tokens:
			c = int(c)
			v = self._children[u].get(c) if u != DEAD else None
			if v is not None:
				total += w
				u, k = v, (0 if self._tables[2][v] else k + 1)
			else:
				v = self._children[0].get(c) if last == self.space else None
				total += -(w * k)
				if v is not None:
					total += w
					u, k = v, (0 if self._tables[2][v] else 1)
				else:
					u, k = (0 if c == self.space else DEAD), 0
			last = c
		return total + -(w * k)


def read_phrases(path):
	"""One phrase per line; blank lines are skipped."""
	with open(path, encoding = 'utf-8') as f:
		return [line.strip() for line in f if line.strip()]
