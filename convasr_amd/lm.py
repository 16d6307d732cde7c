"""n-gram language models for the LM-fused CTC beam search (include/convasr_hip.h: convasr_ctc_beam_search_lm).

The reference's decoders.BeamSearchDecoder scores words with a KenLM model through ctcdecode.  Here the model is read from an ARPA text
file (the exchange format KenLM also reads) and turned into flat tables the kernel looks up:

* read_arpa(path) -> Arpa: the order and every n-gram (a tuple of words) -> (log10 p, log10 backoff weight; 0 when missing).
* NgramLM(arpa_or_path, labels): the vocabulary V (the unigrams other than <s>, </s>, <unk> whose characters all map to labels other
  than the blank and the space) as a trie keyed on label classes, and the n-grams as a table the kernel can search.

Device tables (uploaded once per device by NgramLM.device_tables):
  node_mask  (n_nodes, MW) uint32, MW = ceil(C / 32): bit c set when the node has a child by class c (node 0 is the root = empty word)
  node_child (n_nodes,) int32: the node id of the node's first child; the child by class c is node_child + (number of set bits below c)
  node_word  (n_nodes,) int32: the word id of the word the node ends, -1 when none
  ent_pb     (n_ent, 2) float64: (log10 p, log10 bow) of n-gram entry e; the unigram entry of word w is e = w
  ent_sl     (n_ent, 2) int32: (state id of the longest listed proper suffix of the n-gram (-1: the empty context), n-gram order)
  slots      (n_slots, 4) int32: open-addressing table (linear probing, n_slots a power of two) of every entry of order >= 2 by its full key
             (context entry id, last word id) -> entry id; empty slots hold (-2, -2, -1, 0).  A lookup compares both key fields, so a
             hash collision never yields a false hit.
An LM state is the entry id of the longest suffix of a prefix's word history (at most order - 1 words, <s> in front of a short one)
that the model lists, -1 for the empty context; that state determines every conditional probability of the next word, because an
n-gram is accepted only when its context (its first n - 1 words) is listed too."""
import math
import os
import time

import numpy as np

SPECIAL = ('<s>', '</s>', '<unk>')
MAX_ORDER = 6
EMPTY_KEY = -2


class Arpa:
	def __init__(self, order, ngrams, words):
		self.order = order      # N_lm
		self.ngrams = ngrams    # tuple of words -> (log10 p, log10 bow)
		self.words = words      # the unigrams, in file order (word id = index)


class NotArpaError(NotImplementedError):
	pass


def _not_arpa(path, why):
	return NotArpaError(f'language-model file {path!r} cannot be read as an ARPA text file ({why}): only ARPA language models are supported (no KenLM binary)')


def read_arpa(path):
	"""Parse an ARPA file.  A path that cannot be read as ARPA text at all (missing, unreadable, binary, no \\data\\ header) raises
	NotArpaError (a NotImplementedError); a file with an ARPA header but malformed content raises ValueError naming the line."""
	try:
		with open(path, 'rb') as f:
			raw = f.read()
	except OSError as e:
		raise _not_arpa(path, e.strerror or type(e).__name__) from None
	try:
		text = raw.decode('utf-8')
	except UnicodeDecodeError:
		raise _not_arpa(path, 'not UTF-8 text') from None
	lines = text.split('\n')
	i, n = 0, len(lines)
	while i < n and not lines[i].strip():
		i += 1
	if i >= n or lines[i].strip() != '\\data\\':
		raise _not_arpa(path, 'no \\data\\ header')
	i += 1

	def bad(k, why):
		return ValueError(f'{path}:{k + 1}: malformed ARPA file: {why}')

	counts = {}
	while i < n and lines[i].strip():
		s = lines[i].strip()
		if not s.startswith('ngram ') or '=' not in s:
			raise bad(i, f'expected "ngram N=count" in \\data\\, got {s!r}')
		try:
			k, c = (int(x) for x in s[6:].split('='))
		except ValueError:
			raise bad(i, f'expected "ngram N=count", got {s!r}') from None
		if k != len(counts) + 1 or c < 0:
			raise bad(i, f'n-gram counts must be listed for orders 1, 2, ... with a count >= 0, got {s!r}')
		counts[k] = c
		i += 1
	order = len(counts)
	if not 1 <= order <= MAX_ORDER:
		raise ValueError(f'{path}: ARPA model of order {order}; orders 1 to {MAX_ORDER} are supported')
	if counts[1] < 1:
		raise ValueError(f'{path}: ARPA model without unigrams')
	ngrams, words = {}, []
	for k in range(1, order + 1):
		while i < n and not lines[i].strip():
			i += 1
		if i >= n or lines[i].strip() != f'\\{k}-grams:':
			raise bad(min(i, n - 1), f'expected \\{k}-grams:')
		i += 1
		got = 0
		while i < n and lines[i].strip() and not lines[i].lstrip().startswith('\\'):
			f = lines[i].split()
			if len(f) not in (k + 1, k + 2):
				raise bad(i, f'a {k}-gram entry has {len(f)} fields')
			try:
				p = float(f[0])
				bow = float(f[k + 1]) if len(f) == k + 2 else 0.0
			except ValueError:
				raise bad(i, f'not a number in {lines[i].strip()!r}') from None
			if not (math.isfinite(p) and math.isfinite(bow)):
				raise bad(i, 'non-finite log-probability or backoff weight')
			key = tuple(f[1:k + 1])
			if key in ngrams:
				raise bad(i, f'duplicate n-gram {" ".join(key)!r}')
			if k > 1 and key[:-1] not in ngrams:
				raise bad(i, f'the context {" ".join(key[:-1])!r} of {" ".join(key)!r} is not listed')
			ngrams[key] = (p, bow)
			if k == 1:
				words.append(key[0])
			got += 1
			i += 1
		if got != counts[k]:
			raise bad(i if i < n else n - 1, f'{got} {k}-grams listed, the header says {counts[k]}')
	while i < n and not lines[i].strip():
		i += 1
	if i >= n or lines[i].strip() != '\\end\\':
		raise bad(min(i, n - 1), 'expected \\end\\')
	return Arpa(order, ngrams, words)


def _hash(ctx, word):
	"""The slot hash of the key (context entry id, word id); uint32 arithmetic, the kernel's bs_lm_hash."""
	ctx = np.asarray(ctx).astype(np.uint32)
	word = np.asarray(word).astype(np.uint32)
	with np.errstate(over = 'ignore'):
		h = (ctx * np.uint32(0x9E3779B1)) ^ (word * np.uint32(0x85EBCA77))
		h ^= h >> np.uint32(15)
		h *= np.uint32(0x2C1B3C6D)
		h ^= h >> np.uint32(12)
	return h


def parse_labels(labels):
	"""The reference's list(str(labels).lower()): one character per class."""
	return list(str(labels).lower())


class NgramLM:
	"""An ARPA model bound to a label set.  arpa: a path or an Arpa; labels: one character per class (lowercased).  With this model the
	labels need exactly one space, which is not the blank (checked by the decoder, which knows the blank)."""

	def __init__(self, arpa, labels):
		t0 = time.perf_counter()
		self.path = arpa if isinstance(arpa, (str, os.PathLike)) else None
		self.arpa = read_arpa(arpa) if self.path is not None else arpa
		self.parse_seconds = time.perf_counter() - t0
		self.labels = parse_labels(labels)
		self.num_classes = len(self.labels)
		if self.labels.count(' ') != 1:
			raise ValueError(f'NgramLM: the labels need exactly one space class, got {self.labels.count(" ")}')
		self.space = self.labels.index(' ')
		self.order = self.arpa.order
		cls = {}
		for c, ch in enumerate(self.labels):
			cls.setdefault(ch, c)
		self.char_class = cls
		self._device = {}
		t0 = time.perf_counter()
		self._build()
		self.build_seconds = time.perf_counter() - t0

	def vocabulary_of(self, blank):
		"""V for a given blank class: word -> tuple of classes."""
		bad = {blank, self.space}
		out = {}
		for w in self.arpa.words:
			if w in SPECIAL:
				continue
			cs = tuple(self.char_class.get(ch, -1) for ch in w)
			if cs and all(c >= 0 and c not in bad for c in cs):
				out[w] = cs
		return out

	def _build(self):
		ar = self.arpa
		self.word_id = {w: i for i, w in enumerate(ar.words)}
		# n-gram entries: unigrams first (entry id = word id), then orders 2.. in file order
		keys = [(w,) for w in ar.words] + [k for k in ar.ngrams if len(k) > 1]
		self.entry_id = {k: e for e, k in enumerate(keys)}
		self._keys = keys
		n_ent = len(keys)
		pb = np.empty((n_ent, 2), dtype = np.float64)
		sl = np.empty((n_ent, 2), dtype = np.int32)
		hk_ctx, hk_word, hk_id = [], [], []
		eid = self.entry_id
		for e, k in enumerate(keys):
			pb[e] = ar.ngrams[k]
			suf = -1
			for j in range(1, len(k)):
				s = eid.get(k[j:])
				if s is not None:
					suf = s
					break
			sl[e] = (suf, len(k))
			if len(k) > 1:
				hk_ctx.append(eid[k[:-1]]); hk_word.append(self.word_id[k[-1]]); hk_id.append(e)
		self.ent_pb, self.ent_sl = pb, sl
		m = len(hk_id)
		n_slots = 1
		while n_slots < 2 * m + 2:
			n_slots <<= 1
		slots = np.zeros((n_slots, 4), dtype = np.int32)
		slots[:, 0] = EMPTY_KEY; slots[:, 1] = EMPTY_KEY; slots[:, 2] = -1
		if m:
			hc, hw, hi = np.array(hk_ctx, dtype = np.int64), np.array(hk_word, dtype = np.int64), np.array(hk_id, dtype = np.int64)
			pos = (_hash(hc, hw) & np.uint32(n_slots - 1)).astype(np.int64)
			todo = np.arange(m)
			used = np.zeros(n_slots, dtype = bool)
			while len(todo):  # linear probing, vectorised: per round the first entry aiming at a free slot takes it, the rest move on
				p = pos[todo]
				free = ~used[p]
				first = np.zeros(len(todo), dtype = bool)
				fi = np.nonzero(free)[0]
				_, u = np.unique(p[fi], return_index = True)
				first[fi[u]] = True
				won = todo[first]
				used[pos[won]] = True
				slots[pos[won], 0] = hc[won]; slots[pos[won], 1] = hw[won]; slots[pos[won], 2] = hi[won]
				rest = todo[~first]
				pos[rest] = (pos[rest] + 1) & (n_slots - 1)
				todo = rest
		self.slots = slots
		self.start_state = eid.get(('<s>',), -1) if self.order >= 2 else -1

	def tables(self, blank):
		"""The trie for a given blank (cached): (node_mask, node_child, node_word)."""
		key = ('trie', blank)
		if key in self._device:
			return self._device[key]
		V = self.vocabulary_of(blank)
		if not V:
			raise ValueError('NgramLM: no unigram of the model can be spelled with the labels (other than the blank and the space): the vocabulary is empty')
		if all(len(cs) == 1 for cs in V.values()):
			raise NotImplementedError('NgramLM: every word of the vocabulary is a single character: the character-LM mode of ctcdecode is not supported')
		# trie, breadth-first, children sorted by class: nodes of one parent are contiguous
		children = [{}]
		word_at = [-1]
		for w, cs in V.items():
			nd = 0
			for c in cs:
				nx = children[nd].get(c)
				if nx is None:
					nx = children[nd][c] = len(children)
					children.append({}); word_at.append(-1)
				nd = nx
			word_at[nd] = self.word_id[w]
		C, MW = self.num_classes, (self.num_classes + 31) // 32
		n = len(children)
		order, remap = [0], {0: 0}
		head = 0
		first_child = np.zeros(n, dtype = np.int32)
		while head < len(order):
			old = order[head]
			first_child[head] = len(order)
			for c in sorted(children[old]):
				remap[children[old][c]] = len(order)
				order.append(children[old][c])
			head += 1
		mask = np.zeros((n, MW), dtype = np.uint32)
		word = np.full(n, -1, dtype = np.int32)
		for new, old in enumerate(order):
			word[new] = word_at[old]
			for c in children[old]:
				mask[new, c >> 5] |= np.uint32(1 << (c & 31))
		self._device[key] = (mask, first_child, word)
		return self._device[key]

	def device_tables(self, blank, device):
		"""The tables as device tensors (uploaded once per device and blank)."""
		import torch
		key = ('dev', blank, str(device))
		if key not in self._device:
			mask, child, word = self.tables(blank)
			t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
			self._device[key] = dict(node_mask = t(mask.view(np.int32)), node_child = t(child), node_word = t(word), ent_pb = t(self.ent_pb),
			                         ent_sl = t(self.ent_sl), slots = t(self.slots))
		return self._device[key]

	def log10_cond(self, context, word):
		"""log10 P(word | context) by the backoff rule, with the context as the kernel sees it: the state of a word history (the host
		form of the kernel's bs_lm_score; used by tests)."""
		s = self.state_of(context)
		w = self.word_id[word]
		acc = 0.0
		while True:
			e = w if s < 0 else self.entry_id.get(self._keys[s] + (word,), -1)
			if e >= 0:
				return acc + float(self.ent_pb[e, 0])
			acc += float(self.ent_pb[s, 1])
			s = int(self.ent_sl[s, 0])

	def state_of(self, history):
		"""The LM state of a word history (a list of words, <s> not included): the longest listed suffix of at most order - 1 words."""
		if self.order == 1:
			return -1
		h = tuple(history)
		h = (('<s>',) + h)[-(self.order - 1):] if len(h) < self.order - 1 else h[-(self.order - 1):]
		for j in range(len(h)):
			e = self.entry_id.get(h[j:])
			if e is not None:
				return e
		return -1
