"""A synthetic ARPA model for the LM tests, generated inside the test run (not committed): order 4 over the legacy Russian alphabet,
n_words distinct words of 2-8 letters, and bigrams / trigrams / 4-grams that each extend an n-gram listed one order lower, so every
context is listed.  Deterministic for a given seed."""
import numpy as np

ALPHABET = 'абвгдеёжзийклмнопрстуфхцчшщъыьэюя'


def write(path, n_words = 100_000, n2 = 100_000, n3 = 60_000, n4 = 30_000, seed = 0):
	rng = np.random.default_rng(seed)
	letters = np.array(list(ALPHABET))
	words, seen = [], set()
	while len(words) < n_words:
		lens = rng.integers(2, 9, size = 2 * (n_words - len(words)))
		for L in lens:
			w = ''.join(rng.choice(letters, size = int(L)))
			if w not in seen:
				seen.add(w); words.append(w)
				if len(words) == n_words:
					break
	vocab = ['<unk>', '<s>', '</s>'] + words
	V = len(vocab)
	p1 = -rng.uniform(1.0, 6.0, size = V)
	p1[1] = -99.0
	grams = [[(w,) for w in vocab]]
	for n, count in ((2, n2), (3, n3), (4, n4)):
		prev = grams[-1] if n > 2 else [g for g in grams[0] if g[0] not in ('</s>', '<unk>')]
		out, have = [], set()
		idx = rng.integers(0, len(prev), size = 3 * count)
		nxt = rng.integers(3, V, size = 3 * count)
		for i, j in zip(idx, nxt):
			g = prev[i] + (vocab[j],)
			if g not in have:
				have.add(g); out.append(g)
				if len(out) == count:
					break
		grams.append(out)
	with open(path, 'w', encoding = 'utf-8') as f:
		f.write('\\data\\\n' + ''.join(f'ngram {k + 1}={len(g)}\n' for k, g in enumerate(grams)) + '\n')
		for k, g in enumerate(grams):
			f.write(f'\\{k + 1}-grams:\n')
			ps = p1 if k == 0 else -rng.uniform(0.05, 3.0, size = len(g))
			bows = -rng.uniform(0.0, 1.0, size = len(g))
			has_bow = rng.random(len(g)) < (0.0 if k == len(grams) - 1 else 0.7)
			f.write(''.join(f'{ps[i]:.6f}\t{" ".join(x)}' + (f'\t{bows[i]:.6f}' if has_bow[i] else '') + '\n' for i, x in enumerate(g)))
			f.write('\n')
		f.write('\\end\\\n')
	return path


SMALL_WORDS = ['да', 'нет', 'кот', 'код', 'дом', 'как', 'так', 'он', 'она', 'мы', 'вы', 'ты', 'я', 'лес', 'лето', 'мама', 'рама', 'мыла']


def write_small(path, order, seed = 0, n_per_order = 40):
	"""A small ARPA model of the given order (1..6) over SMALL_WORDS: every unigram, and n_per_order n-grams per higher order, each extending
	an n-gram listed one order lower; about a third of the entries have no backoff weight."""
	rng = np.random.default_rng(seed)
	vocab = ['<unk>', '<s>', '</s>'] + SMALL_WORDS
	grams = [[(w,) for w in vocab]]
	for n in range(2, order + 1):
		prev = grams[-1] if n > 2 else [g for g in grams[0] if g[0] not in ('</s>', '<unk>')]
		out, have = [], set()
		for _ in range(20 * n_per_order):
			g = prev[int(rng.integers(len(prev)))] + (vocab[int(rng.integers(3, len(vocab)))],)
			if g not in have:
				have.add(g); out.append(g)
				if len(out) == n_per_order:
					break
		grams.append(out)
	with open(path, 'w', encoding = 'utf-8') as f:
		f.write('\\data\\\n' + ''.join(f'ngram {k + 1}={len(g)}\n' for k, g in enumerate(grams)) + '\n')
		for k, g in enumerate(grams):
			f.write(f'\\{k + 1}-grams:\n')
			for x in g:
				p = -99.0 if x == ('<s>',) else -float(rng.uniform(0.1, 3.0))
				bow = f'\t{-float(rng.uniform(0.0, 1.0)):.6f}' if k < order - 1 and rng.random() < 0.66 else ''
				f.write(f'{p:.6f}\t{" ".join(x)}{bow}\n')
			f.write('\n')
		f.write('\\end\\\n')
	return path
