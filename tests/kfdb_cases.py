"""Constructed databases for the KeyFrameDatabase queries, shared by tests/test_second_reading_kfdb_cpu.py, tests/test_kfdb_facade_cpu.py
and tests/test_gpu_kfdb.py.  Plain numpy; BowVector rows are made by the second reading of DBoW2 (second_reading_frame) from (word, weight)
features, so that their values are what Frame::ComputeBoW gives.  Imports no product code and no oracle.

A Case is plain data: the database rows in add order (ids, values), which rows were erased, one query, the connected set, and what the
covisibility step reads: a map per row, the ordered covisibility lists, stale members and bad flags."""
import numpy as np

import frame_cases
import second_reading_frame as srf
import second_reading_kfdb as srk

NWORDS = 40000
PRIVATE = 20000                                   # words >= PRIVATE never appear in a query: rows pad their length with them
QUERY_ID = 7
MAX_COMMONS = (1, 4, 5, 6, 10, 15, 99, 100, 101)
ROW_LENGTHS = (0, 1, 63, 64, 65, 129)
ROW_COUNTS = (1, 64, 65, 1000)
MAGNITUDES = [float(w) for w in frame_cases.magnitudes_tree()["weight"][1:]]     # 20 weights over 18 decades


def bow_row(words, weights):
    """The BowVector of features (word, weight) in feature order -> (ids, values)."""
    ids, vals, _, _ = srf.bow_and_feature_vector(list(words), [0] * len(words), list(weights))
    return ids, vals


class Case:
    def __init__(self, name, seed):
        self.name, self.rng = name, np.random.default_rng(seed)
        self.rows, self.active = [], []
        self.query = None
        self.exclude = None                       # per row, the connected set of DetectNBestCandidates; None = empty
        self.n_candidates = 3
        self._private = PRIVATE

    def weights(self, n, magnitudes=False):
        if magnitudes:
            return [MAGNITUDES[i] for i in self.rng.integers(0, len(MAGNITUDES), n)]
        return [float(x) for x in self.rng.uniform(0.1, 9.0, n)]

    def private(self, n):
        out = list(range(self._private, self._private + n))
        self._private += n
        assert self._private <= NWORDS
        return out

    def add_row(self, shared, length=None, active=True, magnitudes=False):
        """A row holding the words `shared` and private words up to `length` entries."""
        words = list(shared) + self.private(max(0, (length or len(shared)) - len(shared)))
        order = self.rng.permutation(len(words))                            # features arrive in any order
        words = [words[i] for i in order]
        self.rows.append(bow_row(words, self.weights(len(words), magnitudes)))
        self.active.append(bool(active))
        return len(self.rows) - 1

    def set_query(self, words, magnitudes=False):
        words = [words[i] for i in self.rng.permutation(len(words))]
        self.query = bow_row(words, self.weights(len(words), magnitudes))

    def finish(self):
        """What the covisibility step reads, seeded: three maps (map 2 is bad), up to 12 neighbours per row, stale members."""
        rng, n = self.rng, len(self.rows)
        self.map_of = [int(x) for x in rng.integers(0, 3, n)]
        self.map_bad = [False, False, True]
        self.query_map = 0
        self.covisible = [[int(x) for x in rng.choice(n, min(n, int(rng.integers(0, 13))), replace=False)] for _ in range(n)]
        self.stale_score = [np.float32(x) for x in rng.uniform(0.0, 0.3, n)]
        self.stale_words = [int(x) for x in rng.integers(0, 50, n)]
        self.bad = [False] * n
        if self.exclude is None:
            self.exclude = [False] * n
        assert len(self.exclude) == n and self.query is not None
        return self

    # the pools as arrays ---------------------------------------------------------------------------------------------
    def pool(self, cap):
        """db_word, db_val [nrows][cap], db_n, db_active.  Unused slots hold -1 / NaN: a reader that leaves a row's length would show."""
        n = len(self.rows)
        word = np.full((n, cap), -1, np.int32); val = np.full((n, cap), np.nan, np.float64); cnt = np.zeros(n, np.int32)
        for r, (ids, vals) in enumerate(self.rows):
            assert len(ids) <= cap
            word[r, :len(ids)] = ids; val[r, :len(ids)] = vals; cnt[r] = len(ids)
        return word, val, cnt, np.array(self.active, np.uint8)

    def query_pool(self, cap):
        ids, vals = self.query
        word = np.full((1, cap), -1, np.int32); val = np.full((1, cap), np.nan, np.float64)
        word[0, :len(ids)] = ids; val[0, :len(ids)] = vals
        return word, val, np.array([len(ids)], np.int32)

    def max_len(self):
        return max([len(self.query[0])] + [len(ids) for ids, _ in self.rows] + [1])


def build(case, place):
    """The second reading's objects of a case: (database, rows in add order, query, maps).  place = DetectNBestCandidates' members."""
    maps = [srk.Map(bad) for bad in case.map_bad]
    rows = [srk.KeyFrame(ids, vals, maps[case.map_of[r]], case.bad[r]) for r, (ids, vals) in enumerate(case.rows)]
    db = srk.KeyFrameDatabase(NWORDS)
    for r, kf in enumerate(rows):
        kf.covisible = [rows[c] for c in case.covisible[r]]
        kf.mRelocScore = kf.mPlaceRecognitionScore = case.stale_score[r]
        kf.mnRelocWords = kf.mnPlaceRecognitionWords = case.stale_words[r]
        db.add(kf)
    for r, kf in enumerate(rows):
        if not case.active[r]:
            db.erase(kf)
    if place:
        query = srk.KeyFrame(case.query[0], case.query[1], maps[case.query_map])
        query.mnId = 1000000 + QUERY_ID
        query.connected = {rows[r] for r in range(len(rows)) if case.exclude[r]}
    else:
        query = srk.Frame(case.query[0], case.query[1], QUERY_ID)
    return db, rows, query, maps


def expected(case, place):
    """The eight outputs of the device query for the case, from the second reading (see second_reading_kfdb.query_rows)."""
    db, rows, query, _ = build(case, place)
    out = srk.query_rows(db, rows, query, case.exclude if place else None, place)
    out["branches"] = db.t
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def _max_common_case(m):
    """The largest row shares m words; one row shares exactly min_common = (int)(m * 0.8f) words and one min_common + 1."""
    c = Case("max_common_%d" % m, 100 + m)
    q = list(range(10, 10 + m + 7))
    c.set_query(q)
    mn = int(np.float32(m) * np.float32(0.8))
    c.add_row(q[:min(3, max(1, m // 2))], 12)
    c.add_row(q[:m], m + 5)                                                # the maximum
    c.add_row(q[2:2 + mn], mn + 9)                                           # exactly min_common: not scored (strict >); shares nothing when it is 0
    if mn + 1 <= m:
        c.add_row(q[1:2 + mn], mn + 4)                                       # min_common + 1: scored
    c.add_row([], 6)
    return c.finish()


def _row_lengths_case():
    """Row lengths 0, 1, 63, 64, 65, 129; the shared word is the row's first entry, its last, or the query's last only."""
    c = Case("row_lengths", 7)
    q = list(range(1000, 1040))
    c.set_query(q + [PRIVATE - 1])                                           # the query's last word, above every other query word
    for n in ROW_LENGTHS:
        c.add_row(q[:min(n, 5)], n)                                          # the shared words are the row's first entries (private words are larger)
    for n in ROW_LENGTHS[1:]:
        c.add_row([PRIVATE - 1], n)                                          # shares the query's last word only
    for n in ROW_LENGTHS[1:]:
        low = [int(x) for x in c.rng.choice(900, n - 1, replace=False)]      # words below every query word: the shared word is the row's LAST entry
        c.rows.append(bow_row(low + [q[7]], c.weights(n))); c.active.append(True)
    return c.finish()


def _row_count_case(nrows):
    c = Case("rows_%d" % nrows, 900 + nrows)
    q = [int(x) for x in np.sort(c.rng.choice(PRIVATE, 120, replace=False))]
    c.set_query(q)
    for r in range(nrows):
        k = int(c.rng.integers(0, 40)) if r else 17
        shared = [q[i] for i in np.sort(c.rng.choice(len(q), k, replace=False))]
        c.add_row(shared, k + int(c.rng.integers(0, 30)), active=bool(c.rng.random() > 0.05) or r == 0)
    return c.finish()


def _identical_case():
    c = Case("identical_row", 11)
    q = list(range(500, 570))
    c.set_query(q)
    c.add_row(q[:30], 40)
    c.rows.append((c.query[0].copy(), c.query[1].copy())); c.active.append(True)         # the query itself: score (float)1.0 up to the sum's rounding
    c.add_row(q[60:], 20)
    return c.finish()


def _no_sharing_case():
    c = Case("no_sharing", 12)
    c.set_query(list(range(300, 330)))
    for n in (5, 64, 0):
        c.add_row([], n)
    return c.finish()


def _masked_maximum_case():
    """An erased row and a connected row would each hold the maximum."""
    c = Case("masked_maximum", 13)
    q = list(range(700, 760))
    c.set_query(q)
    c.add_row(q[:50], 70, active=False)
    c.add_row(q[:45], 50)                                                    # connected: excluded in the place-recognition form only
    c.add_row(q[:10], 30)
    c.add_row(q[:9], 30)
    c.add_row(q[:8], 30)
    c.add_row(q[3:6], 10)
    c.exclude = [False, True, False, False, False, False]
    return c.finish()


def _same_first_word_case():
    """Rows 1 and 3 enter the list at one word, row 2 at an earlier one, row 0 at a later one: the list is 2, 1, 3, 0."""
    c = Case("same_first_word", 14)
    q = list(range(40, 60))
    c.set_query(q)
    c.add_row(q[9:12], 6)
    c.add_row(q[4:9], 9)
    c.add_row(q[1:3], 4)
    c.add_row([q[4], q[15], q[16], q[17], q[18]], 8)
    return c.finish()


def _magnitudes_case():
    """Values over 18 decades: the order of L1Scoring's sum decides its last bits."""
    c = Case("magnitudes", 15)
    q = list(range(2000, 2150))
    c.set_query(q, magnitudes=True)
    for k in (150, 149, 140, 130, 125, 121, 120, 64, 65):
        c.add_row(q[:k], k + 3, magnitudes=True)
    return c.finish()


_MAKERS = {"row_lengths": _row_lengths_case, "identical_row": _identical_case, "no_sharing": _no_sharing_case,
           "masked_maximum": _masked_maximum_case, "same_first_word": _same_first_word_case, "magnitudes": _magnitudes_case}
_MAKERS.update({"max_common_%d" % m: (lambda m=m: _max_common_case(m)) for m in MAX_COMMONS})
_MAKERS.update({"rows_%d" % n: (lambda n=n: _row_count_case(n)) for n in ROW_COUNTS})
CASE_NAMES = tuple(_MAKERS)
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _MAKERS[name]()
        assert _CASES[name].name == name
    return _CASES[name]


def random_case(seed):
    """A seeded random database for the covisibility step: 5..60 rows over a small vocabulary, so that many rows share words, scores tie
    (identical rows) and neighbours are often sharing but not scored."""
    c = Case("random_%d" % seed, 5000 + seed)
    rng = c.rng
    vocab = int(rng.integers(20, 200))
    q = [int(x) for x in np.sort(rng.choice(vocab, int(rng.integers(1, min(vocab, 40))), replace=False))]
    c.set_query(q)
    nrows = int(rng.integers(5, 61))
    for r in range(nrows):
        if r and rng.random() < 0.15:
            src = int(rng.integers(0, r))
            c.rows.append(c.rows[src]); c.active.append(True)                # a twin: equal scores
            continue
        k = int(rng.integers(0, min(vocab, 30)))
        words = [int(x) for x in rng.choice(vocab, k, replace=False)]
        c.add_row(words, k + int(rng.integers(0, 4)), active=bool(rng.random() > 0.1))
    c.exclude = [bool(rng.random() < 0.1) for _ in range(nrows)]
    c.n_candidates = int(rng.integers(1, 5))
    return c.finish()


def big_case():
    """The largest shape of the GPU test: 4096 rows of up to 256 words."""
    c = Case("big_4096x256", 4096)
    rng = c.rng
    q = np.sort(rng.choice(PRIVATE, 256, replace=False))
    c.query = bow_row([int(x) for x in q], c.weights(256))
    pool = np.arange(PRIVATE)
    for r in range(4096):
        n = int(rng.integers(1, 257))
        k = min(n, int(rng.integers(0, 60)))
        words = np.concatenate([rng.choice(q, k, replace=False), rng.choice(pool, n - k, replace=False)])
        words = np.unique(words)
        w = rng.uniform(0.1, 9.0, len(words))
        c.rows.append((words.astype(np.int32), w / w.sum())); c.active.append(bool(rng.random() > 0.02))
    return c.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# part 1: (word, weight) feature rows for orbm_bow_vector_batch_async
# ---------------------------------------------------------------------------------------------------------------------------
BOWVEC_COUNTS = (0, 1, 63, 64, 65)
BOWVEC_CAPS = (67, 1000)


def bow_vector_rows(cap):
    """-> list of (name, word_id [count], weight [count]) with count <= cap."""
    rng = np.random.default_rng(cap)
    out = []
    mag = np.array(MAGNITUDES)
    for n in BOWVEC_COUNTS + ((cap,) if cap not in BOWVEC_COUNTS else ()):
        out.append(("one_word_%d" % n, np.full(n, 5, np.int32), mag[rng.integers(0, len(mag), n)]))      # one run: the sum's order decides
        out.append(("all_distinct_%d" % n, rng.permutation(3 * n + 1)[:n].astype(np.int32), mag[rng.integers(0, len(mag), n)]))
        out.append(("all_stopped_%d" % n, rng.integers(0, 9, n).astype(np.int32), np.zeros(n)))
        w = rng.uniform(0.1, 9.0, n)
        kind = rng.integers(0, 6, n)
        w[kind == 0] = 0.0; w[kind == 1] = -w[kind == 1]; w[kind == 2] = np.nan
        out.append(("mixed_%d" % n, rng.integers(0, max(2, n // 3), n).astype(np.int32), w))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the text form tests/kfdb_facade.cpp reads, and what the second reading says it must print
# ---------------------------------------------------------------------------------------------------------------------------
def _bow_text(ids, vals):
    bits = np.ascontiguousarray(vals, np.float64).view(np.uint64)
    return "%d %s %s" % (len(ids), " ".join(str(int(i)) for i in ids), " ".join(str(int(b)) for b in bits))


def facade_text(items):
    """items: (case, place, rows) with rows = the query's common / first_word / score arrays (the device's, or the second reading's)."""
    lines = [str(len(items))]
    for c, place, rows in items:
        n = len(c.rows)
        qid = 1000000 + QUERY_ID if place else QUERY_ID
        lines.append("%d %d %d %d %d %d %d" % (int(place), n, qid, c.query_map, c.n_candidates, len(c.map_bad), c.max_len()))
        lines.append(" ".join(str(int(b)) for b in c.map_bad))
        lines.append(_bow_text(*c.query))
        for r in range(n):
            lines.append("%d %d %d %d %d %d %d %s" % (c.map_of[r], int(c.bad[r]), int(c.active[r]), int(c.exclude[r]) if place else 0, c.stale_words[r],
                                                      int(np.float32(c.stale_score[r]).view(np.uint32)), len(c.covisible[r]),
                                                      " ".join(str(x) for x in c.covisible[r])))
            lines.append(_bow_text(*c.rows[r]))
        lines.append(" ".join(str(int(x)) for x in rows["common"]))
        lines.append(" ".join(str(int(x)) for x in rows["first_word"]))
        lines.append(" ".join(str(int(x)) for x in np.ascontiguousarray(rows["score"], np.float32).view(np.uint32)))
    return "\n".join(lines) + "\n"


def facade_expected(c, place):
    """The second reading end to end -> (lists of row indices, per row (query, words, score bits) afterwards)."""
    db, rows, query, maps = build(c, place)
    index = {id(kf): r for r, kf in enumerate(rows)}
    if place:
        loop, merge = db.detect_n_best_candidates(query, c.n_candidates)
        lists = {"L": [index[id(k)] for k in loop], "M": [index[id(k)] for k in merge]}
        members = [(kf.mnPlaceRecognitionQuery, kf.mnPlaceRecognitionWords, int(np.float32(kf.mPlaceRecognitionScore).view(np.uint32))) for kf in rows]
    else:
        out = db.detect_relocalization_candidates(query, maps[c.query_map])
        lists = {"R": [index[id(k)] for k in out]}
        members = [(kf.mnRelocQuery, kf.mnRelocWords, int(np.float32(kf.mRelocScore).view(np.uint32))) for kf in rows]
    return lists, members, db.t


def parse_facade_output(text, items):
    """-> per item (lists, members) in the shape of facade_expected."""
    lines = text.strip().split("\n")
    out, pos = [], 0
    for i, (c, place, _) in enumerate(items):
        tok = lines[pos].split(); pos += 1
        assert tok[:2] == ["case", str(i)], lines[pos - 1]
        lists, k = {}, 2
        while k < len(tok):
            n = int(tok[k + 1])
            lists[tok[k]] = [int(x) for x in tok[k + 2:k + 2 + n]]
            k += 2 + n
        members = [tuple(int(x) for x in lines[pos + r].split()) for r in range(len(c.rows))]
        pos += len(c.rows)
        out.append((lists, members))
    return out


def check_facade(got, c, place):
    """The facade's lists equal the second reading's; so do the members, but for mnPlaceRecognitionWords of a connected KeyFrame, which
    the facade leaves alone and nobody reads (facade/KeyFrameDatabase.h)."""
    lists, members, _ = facade_expected(c, place)                          # _ = the branches taken
    assert got[0] == lists, (c.name, place, got[0], lists)
    for r, (g, w) in enumerate(zip(got[1], members)):
        if place and c.exclude[r]:
            assert g[0] == w[0] and g[2] == w[2], (c.name, r, g, w)
        else:
            assert g == w, (c.name, place, r, g, w)
    return _
