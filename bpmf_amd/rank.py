"""Ranked evaluation: the host side of `gibbs(..., rank_eval=N)` -- the held-out lists engine.rank_eval
takes, built from a test matrix, and the metrics of the ranks it returns.  Plain numpy."""
import numpy as np


def held_out_lists(T, nqueries, by="rows", threshold=None):
    """The held-out candidates of every query from the test matrix T = (colptr, rowidx, vals), CSC with one column per movie and
    the users as rows.  by="rows": the users are the queries and the movies the candidates; by="cols": the other way round.
    threshold: only the cells with a value > threshold are held-out items (None: every cell).
    Returns (tptr int64[nqueries + 1], tcand int32[n], cell int64[n]): query q holds out tcand[tptr[q] : tptr[q + 1]], ascending, and
    entry p is cell cell[p] of T in its order.  ValueError: a cell is listed twice."""
    if by not in ("rows", "cols"):
        raise ValueError("rank_by must be 'rows' or 'cols', not %r" % (by,))
    colptr = np.asarray(T[0], np.int64)
    rows = np.asarray(T[1], np.int64)
    vals = np.asarray(T[2], np.float64)
    cols = np.repeat(np.arange(len(colptr) - 1, dtype=np.int64), np.diff(colptr))
    q, c = (rows, cols) if by == "rows" else (cols, rows)
    cell = np.arange(len(rows), dtype=np.int64)
    if threshold is not None:
        keep = vals > float(threshold)
        q, c, cell = q[keep], c[keep], cell[keep]
    if len(q) and (q.min() < 0 or q.max() >= nqueries):
        raise ValueError("held_out_lists: the test matrix names query %d of %d" % (int(q.max()), nqueries))
    order = np.lexsort((c, q))
    q, c, cell = q[order], c[order], cell[order]
    same = (q[1:] == q[:-1]) & (c[1:] == c[:-1])
    if same.any():
        p = int(np.argmax(same))
        raise ValueError("held_out_lists: the test cell (query %d, candidate %d) is listed twice" % (int(q[p]), int(c[p])))
    tptr = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=nqueries))]).astype(np.int64)
    return tptr, np.ascontiguousarray(c, np.int32), cell


def rank_metrics(rank, tptr, ncand, n):
    """Metrics at list length n of the ranks engine.rank_eval returns.  rank[p] >= 1: the rank of held-out entry p among the ncand[q]
    candidates its query q has not rated; tptr: the entries of query q are tptr[q] : tptr[q + 1].  With h_q the number of held-out
    entries of query q, Q the queries with h_q > 0, and every mean taken over what is named (NaN when that is empty):

      recall   mean over Q of  #{p of q : rank[p] <= n} / min(n, h_q)
      ndcg     mean over Q of  DCG_q / IDCG_q with binary gains:  DCG_q = sum over p of q with rank[p] <= n of 1 / log2(1 + rank[p]),
               IDCG_q = sum_{i = 1 .. min(n, h_q)} 1 / log2(1 + i)   (the held-out items first)
      mrr      mean over Q of  1 / min_p rank[p]
      mpr      mean over the ENTRIES with ncand[q] > 1 of  (rank[p] - 1) / (ncand[q] - 1)     (0: first, 1: last)
      auc      mean over the queries of Q with ncand[q] > h_q of the share of (held-out, other) pairs in which the held-out entry
               comes first: with the query's ranks sorted ascending, r_(1) < ... < r_(h), entry i has r_(i) - i other candidates
               before it, so the share is  1 - sum_i (r_(i) - i) / (h_q (ncand[q] - h_q))
      queries  |Q|
      entries  the number of held-out entries

    The held-out entries of a query count each other as candidates, so their ranks are distinct."""
    rank = np.asarray(rank, np.int64)
    tptr = np.asarray(tptr, np.int64)
    ncand = np.asarray(ncand, np.int64)
    n = int(n)
    if n < 1:
        raise ValueError("rank_metrics: n must be >= 1")
    if tptr.ndim != 1 or len(tptr) != len(ncand) + 1 or (len(tptr) and (tptr[0] != 0 or int(tptr[-1]) != len(rank))) or np.any(np.diff(tptr) < 0):
        raise ValueError("rank_metrics: tptr must run from 0 to len(rank) over len(ncand) queries")
    if len(rank) and rank.min() < 1:
        raise ValueError("rank_metrics: a rank below 1")
    nan = float("nan")
    recall, ndcg, mrr, auc = [], [], [], []
    disc = 1.0 / np.log2(2.0 + np.arange(n))                         # 1 / log2(1 + i), i = 1 .. n
    for q in range(len(ncand)):
        r = np.sort(rank[tptr[q]:tptr[q + 1]])
        h = len(r)
        if h == 0:
            continue
        top = r[r <= n]
        recall.append(len(top) / min(n, h))
        ndcg.append(float(np.sum(1.0 / np.log2(1.0 + top))) / float(np.sum(disc[:min(n, h)])))
        mrr.append(1.0 / float(r[0]))
        others = int(ncand[q]) - h
        if others > 0:
            before = r - np.arange(1, h + 1)
            auc.append(1.0 - float(before.sum()) / (h * others))
    nq_of = np.repeat(ncand, np.diff(tptr))
    ok = nq_of > 1
    mpr = float(np.mean((rank[ok] - 1) / (nq_of[ok] - 1))) if ok.any() else nan
    mean = lambda v: float(np.mean(v)) if len(v) else nan
    return dict(recall=mean(recall), ndcg=mean(ndcg), mrr=mean(mrr), mpr=mpr, auc=mean(auc), queries=len(recall), entries=int(len(rank)))
