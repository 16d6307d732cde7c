"""A Python restatement of convasr_nw_align (include/convasr_hip.h): the semi-global Needleman-Wunsch alignment with traceback, written from
its definition.

Two forms: `nw_align_loop`, the plain double loop over the full matrix followed by the walk over the matrix itself, and `nw_align`, a numpy
row DP in which each row's left-to-right dependency M[i][j] = max(E[j], M[i][j-1] + ins) becomes j * ins + a running maximum of
E[k] - k * ins (np.maximum.accumulate), and which keeps 2 direction bits per cell instead of the matrix.  The loop is the definition; tests
check the numpy form against it and use the numpy form for volume.

Both return (a_index, b_index, score): per alignment column, in forward order, the 0-based unit of a / of b or -1 for a gap, and the end
cell's score."""
import numpy as np

WORD_SCORES = (100, -6, -8, -3)  # (match, sub, del, ins) the reference's align_strings runs with at word level
CHAR_SCORES = (5, -3, -4, -3)  # and at character level


def _end_cell(la, lb, last_row, last_col):
	if la < lb:
		j = max(range(lb + 1), key = lambda k: (last_row[k], -k))
		return la, j, last_row[j]
	i = max(range(la + 1), key = lambda k: (last_col[k], -k))
	return i, lb, last_col[i]


def _emit(la, lb, ei, ej, step):
	"""Walks back from (ei, ej); step(i, j) -> 0 (ins), 1 (del) or 2 (diagonal)."""
	cols = [(-1, k) for k in range(ej, lb)] if la < lb else [(k, -1) for k in range(ei, la)]
	cols.reverse()
	i, j = ei, ej
	while i > 0 or j > 0:
		if i == 0 or j == 0:
			cols += [(-1, k) for k in range(j - 1, -1, -1)] if i == 0 else [(k, -1) for k in range(i - 1, -1, -1)]
			break
		d = step(i, j)
		if d == 0:
			cols.append((-1, j - 1))
			j -= 1
		elif d == 1:
			cols.append((i - 1, -1))
			i -= 1
		else:
			cols.append((i - 1, j - 1))
			i, j = i - 1, j - 1
	cols.reverse()
	return [c[0] for c in cols], [c[1] for c in cols]


def nw_align_loop(a, b, scores):
	match, sub, dele, ins = scores
	la, lb = len(a), len(b)
	M = [[0] * (lb + 1) for _ in range(la + 1)]
	for i in range(1, la + 1):
		for j in range(1, lb + 1):
			M[i][j] = max(M[i - 1][j - 1] + (match if a[i - 1] == b[j - 1] else sub), M[i - 1][j] + dele, M[i][j - 1] + ins)
	ei, ej, score = _end_cell(la, lb, M[la], [row[lb] for row in M])
	step = lambda i, j: 0 if M[i][j] == M[i][j - 1] + ins else 1 if M[i][j] == M[i - 1][j] + dele else 2
	return (*_emit(la, lb, ei, ej, step), score)


def nw_align(a, b, scores):
	match, sub, dele, ins = scores
	a, b = np.asarray(a, dtype = np.int64), np.asarray(b, dtype = np.int64)
	la, lb = len(a), len(b)
	k = np.arange(lb + 1, dtype = np.int64) * ins
	row = np.zeros(lb + 1, dtype = np.int64)
	e = np.zeros(lb + 1, dtype = np.int64)
	dirs = np.zeros((la + 1, lb + 1), dtype = np.uint8)
	last_col = [0] * (la + 1)
	for i in range(1, la + 1):
		e[1:] = np.maximum(row[:-1] + np.where(b == a[i - 1], match, sub), row[1:] + dele)
		new = np.maximum.accumulate(e - k) + k
		dirs[i, 1:] = np.where(new[1:] == new[:-1] + ins, 0, np.where(new[1:] == row[1:] + dele, 1, 2))
		row = new
		last_col[i] = int(row[lb])
	ei, ej, score = _end_cell(la, lb, row.tolist(), last_col)
	return (*_emit(la, lb, ei, ej, lambda i, j: int(dirs[i, j])), int(score))
