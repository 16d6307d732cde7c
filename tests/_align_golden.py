"""What the alignment tests share: the golden fixture of the reference's analysis (tests/golden/analysis.json), an aligner and a scorer made of
the Python restatements (tests/_align_ref.py, tests/_metrics_ref.py), and the comparison of an analysis with the fixture."""
import json
import os

import _align_ref as A
import _metrics_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'analysis.json')


WORD_FIELDS = ['_hyp_', '_ref_', 'hyp', 'ref', 'ref_tags', 'hyp_tags', 'error_tags', 'error_tag', 'len', 'cer']
ERROR_TAGS = ['ok', 'typo_easy', 'typo_hard', 'missing', 'missing_ref']
CHAR_STATS = ['ok', 'replace', 'delete', 'insert', 'delete_spaces', 'insert_spaces', 'total_spaces']
CONFIG_FIELDS = ['num_words', 'num_words_ok', 'num_words_missing', 'mer_wordwise', 'wer_wordwise', 'cer_wordwise', 'cer_filtered', 'wer_filtered',
                 'cer_pseudo', 'wer_pseudo', 'ref_vocabness', 'hyp_vocabness']

# The fixture stores every output of the reference without loss, but without repeating what follows from the rest of a record; the script
# that writes it (tests/golden/make_golden_analysis.py) asserts that decoding gives back the reference's own objects.
#   word: [_hyp_, _ref_, ref tag code, hyp tag code, index into ERROR_TAGS, cer], or [word, tag code] where both sides are the same string
#         (then the tags are equal, the error tag is ok and the cer 0); tag code = 1 for vocab_hit (else vocab_miss) + 2 for stop
#   postproc words: a word as above, or the index of an equal word in the case's `words`
#   analysis: cer, wer, chars (CHAR_STATS order), configs (one list in CONFIG_FIELDS order per config); the four texts equal the inputs


def decode_tags(code):
	return ['vocab_hit' if code & 1 else 'vocab_miss'] + (['stop'] if code & 2 else [])


def decode_word(enc):
	_hyp_, _ref_, ref_code, hyp_code, error, cer = enc if len(enc) == 6 else (enc[0], enc[0], enc[1], enc[1], 0, 0)
	hyp, ref = _hyp_.replace('|', ''), _ref_.replace('|', '')
	return dict(zip(WORD_FIELDS, [_hyp_, _ref_, hyp, ref, decode_tags(ref_code), decode_tags(hyp_code), [ERROR_TAGS[error]], ERROR_TAGS[error], len(ref), cer]))


def decode_case(n, enc, config_names):
	words = [decode_word(w) for w in enc['words']]
	analysis = dict(ref = enc['ref'], hyp = enc['hyp'], ref_orig = enc['ref'], hyp_orig = enc['hyp'], cer = enc['cer'], wer = enc['wer'], n = n,
	                char_stats = dict(zip(CHAR_STATS, enc['chars'])), **{c: dict(zip(CONFIG_FIELDS, v)) for c, v in zip(config_names, enc['configs'])})
	return dict(hyp = enc['hyp'], ref = enc['ref'], align_strings = enc['aligned'], align_words = words,
	            align_words_postproc = [dict(words[w]) if isinstance(w, int) else decode_word(w) for w in enc['postproc']], analyze = analysis)


def load_golden():
	"""The fixture, decoded: vocab, stop, configs, cases (hyp, ref, align_strings, align_words, align_words_postproc, analyze: the reference's
	outputs as it returned them, analyze without its 'alignment', which equals align_words) and aggregate."""
	with open(GOLDEN) as f:
		g = json.load(f)
	g['cases'] = [decode_case(n, enc, list(g['configs'])) for n, enc in enumerate(g['cases'])]
	g['aggregate']['errors']['words'] = [g['cases'][c]['align_words'][w] for c, w in g['aggregate']['errors']['words']]
	return g


def ref_aligner(a_seqs, b_seqs, scores):
	return [A.nw_align(a, b, scores)[:2] for a, b in zip(a_seqs, b_seqs)]


def ref_scorer(hyps, refs):
	return [R.cer(h, r) for h, r in zip(hyps, refs)], [R.wer(h, r) for h, r in zip(hyps, refs)]


def words_of(golden, words):
	return [dict(w) for w in words]


def make_analyzer(golden, aligner = ref_aligner, scorer = ref_scorer):
	from convasr_amd import metrics
	tagger = metrics.WordTagger(word_tags = dict(stop = golden['stop']), vocab = set(golden['vocab']))
	return metrics.ErrorAnalyzer(word_tagger = tagger, error_tagger = metrics.ErrorTagger(), configs = golden['configs'], aligner = aligner, scorer = scorer)


def check_analysis(golden, results, aggregate):
	"""results: analyze_batch(detailed = True) over every golden pair, in order; aggregate: the analyzer's aggregate of them."""
	assert len(results) == len(golden['cases'])
	for case, res in zip(golden['cases'], results):
		res = dict(res)
		assert res.pop('alignment') == words_of(golden, case['align_words']), (case['hyp'], case['ref'])
		assert res == case['analyze'], (case['hyp'], case['ref'])
	want = json.loads(json.dumps(golden['aggregate']))
	want['errors']['words'] = words_of(golden, want['errors']['words'])
	aggregate = dict(aggregate, errors = dict(aggregate['errors'], distribution = {str(k): v for k, v in aggregate['errors']['distribution'].items()}))
	assert aggregate == want
