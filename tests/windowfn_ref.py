"""Independent Python restatement of the window functions beyond ROW_NUMBER
(AmdWindowFnConfig in include/arroyo_amd_types.h, restated there from
DataFusion 48): the checker of tests/test_windowfn_funcs.py and
tests/test_windowfn_rank_pipeline.py.  Plain Python integers over one
instant's rows; it imports nothing from the package under test and names
functions and frames by strings of its own.

    layout = Layout(part, orders)            # the sort and the peer groups
    values = layout.values(arg, "lag", k=2)  # [(value, valid)] by position

`part` is a sequence or None, `orders` a list of (sequence, descending).
Positions are sorted positions: partition, ORDER BY columns, arrival."""

FUNCTIONS = ("row_number", "rank", "dense_rank", "lag", "lead",
             "first_value", "last_value", "sum", "count", "min", "max")
FRAMES = ("range", "rows", "partition")
FRAMED = ("first_value", "last_value", "sum", "count", "min", "max")
TAKES_ARG = ("lag", "lead", "first_value", "last_value", "sum", "min", "max")


def wrap64(x):
    """two's-complement i64 of a Python integer"""
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


class Layout:
    def __init__(self, part, orders):
        n = len(orders[0][0])
        part = [0] * n if part is None else [int(p) for p in part]
        keys = [[-int(v) if desc else int(v) for v in col]
                for col, desc in orders]
        rows = sorted(range(n),
                      key=lambda i: (part[i],) + tuple(k[i] for k in keys)
                      + (i,))
        self.n = n
        self.rows = rows          # sorted position -> arrival index
        # per sorted position, all as sorted positions of the instant
        self.p0 = [0] * n         # first row of its partition
        self.p1 = [0] * n         # last row of its partition
        self.g0 = [0] * n         # first row of its peer group (ps)
        self.g1 = [0] * n         # last row of its peer group (pe)
        self.dense = [0] * n
        s = 0
        while s < n:
            e = s
            while e + 1 < n and part[rows[e + 1]] == part[rows[s]]:
                e += 1
            g, dense = s, 0
            while g <= e:
                h = g
                while h + 1 <= e and all(k[rows[h + 1]] == k[rows[g]]
                                         for k in keys):
                    h += 1
                dense += 1
                for t in range(g, h + 1):
                    self.p0[t], self.p1[t] = s, e
                    self.g0[t], self.g1[t] = g, h
                    self.dense[t] = dense
                g = h + 1
            s = e + 1

    def peer_groups(self):
        """(first, last) sorted positions of every peer group"""
        return sorted(set(zip(self.g0, self.g1)))

    def partitions(self):
        return sorted(set(zip(self.p0, self.p1)))

    def values(self, arg, fn, frame="range", k=1, default=None):
        """[(value, valid)] by sorted position; the value under a NULL is
        0.  `arg` is by arrival index (None where fn takes none)."""
        assert fn in FUNCTIONS and frame in FRAMES and k >= 0
        a = None if arg is None else [int(arg[r]) for r in self.rows]
        out = []
        run_sum = run_min = run_max = None   # over p0..t, by position
        sums, mins, maxs = [], [], []
        if fn in ("sum", "min", "max"):
            for t in range(self.n):
                if t == self.p0[t]:
                    run_sum, run_min, run_max = a[t], a[t], a[t]
                else:
                    run_sum += a[t]
                    run_min = min(run_min, a[t])
                    run_max = max(run_max, a[t])
                sums.append(run_sum)
                mins.append(run_min)
                maxs.append(run_max)
        for t in range(self.n):
            p0, p1 = self.p0[t], self.p1[t]
            e = {"rows": t, "range": self.g1[t], "partition": p1}[frame]
            valid = True
            if fn == "row_number":
                v = t - p0 + 1
            elif fn == "rank":
                v = self.g0[t] - p0 + 1
            elif fn == "dense_rank":
                v = self.dense[t]
            elif fn in ("lag", "lead"):
                j = t - k if fn == "lag" else t + k
                if p0 <= j <= p1:
                    v = a[j]
                elif default is not None:
                    v = default
                else:
                    v, valid = 0, False
            elif fn == "first_value":
                v = a[p0]
            elif fn == "last_value":
                v = a[e]
            elif fn == "count":
                v = e - p0 + 1
            elif fn == "sum":
                v = wrap64(sums[e])
            elif fn == "min":
                v = mins[e]
            else:
                v = maxs[e]
            out.append((v, valid))
        return out


def window_rows(cols, part_col, order, fn, arg_col=-1, frame="range", k=1,
                default=None, limit=0):
    """A whole stream: cols = [data columns..., _timestamp] in arrival
    order, order = [(column index, descending)].  Returns the output rows
    (input columns + function value) and the function column's validity,
    instants in timestamp order and each instant's rows in sort order,
    after the `value <= limit` filter."""
    ts = [int(t) for t in cols[-1]]
    by_ts = {}
    for i, t in enumerate(ts):
        by_ts.setdefault(t, []).append(i)
    rows, valid = [], []
    for t in sorted(by_ts):
        idx = by_ts[t]
        lay = Layout(None if part_col < 0 else [cols[part_col][i] for i in idx],
                     [([cols[c][i] for i in idx], d) for c, d in order])
        arg = None if arg_col < 0 else [cols[arg_col][i] for i in idx]
        vals = lay.values(arg, fn, frame, k, default)
        for pos, (v, ok) in enumerate(vals):
            if limit and v > limit:
                continue
            i = idx[lay.rows[pos]]
            rows.append(tuple(int(c[i]) for c in cols) + (v,))
            valid.append(ok)
    return rows, valid
