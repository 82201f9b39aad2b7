"""Hand-built neighbour lists that make the lane groups of the reverse-list collapse (csrc/csr.hip, csr_collapse) own SEVERAL
source points each.  A plain helper module: test_csr_group_cases_host.py asserts on the CPU what test_gpu_csr_groups.py relies
on, and both take the cases from CASES so that neither can drift.

How many consecutive points a lane group owns depends on the number of source points G = B * n alone (plan() below restates
the rule), and the cost of the pass on G * C and on the number of edges: a cloud with very many source points and a few
thousand hand-placed edges reaches every kernel and every `per` in a few hundred MB.

build() does not run a ball query.  Per cloud the targets of idx lie in five windows of 4 * per consecutive source points --
at the start, at 1/4, 1/2 and 3/4, and at the end of the cloud (three windows touch at most 2 * 3 * 5 = 30 lane groups in two
clouds, one of them aligned with point 0: the 30 groups with several lists that the host test asks for need more) -- so that
the lists of one lane group are long, short and empty next to each other:

  * the first and the last point of every cloud are hubs: the lane group that holds a cloud boundary b * n has edges of both
    clouds, whatever the chunk of eight that the boundary falls into;
  * the last cloud's end window lies groups * per + 5 points lower, and nothing else points behind it: the last workgroup has
    points (fewer than it could take) and no edge;
  * of the lane groups that lie wholly inside a window every other one starts (x, empty, y) with x, y taken in turn from
    SLOT_CYCLE -- the list lengths 1, 8, 9, 16, 17 around the kernels' chunks of eight, and hubs -- and the others start with
    two non-empty lists; every remaining point draws a skewed random length int(dmax * u^3), a third of them 0;
  * rows are padded the way a ball query pads them: j distinct targets (1 .. 8), the first of them a hub, the other 32 - j
    slots repeat slot 0.  A hub collects at most HUB_ROWS rows, 32 * HUB_ROWS = 224 edges (LONGEST allows 256);
  * every fifth row is uniform over the cloud's points outside the windows (below the end window in the last cloud): isolated
    one-edge lists among empty ones.
"""
import collections

import numpy as np

# csrc/csr.hip
WGS = 4096        # workgroups csr_pts_per_group() aims at
BS = 256          # CSR_BS: threads of a collapse workgroup
STREAM_PMAX = 16  # CSR_STREAM_PMAX: most points per lane group that the stream kernel takes

K = 32
WINDOW_GROUPS = 4  # a window is this many times `per` points
FRACTIONS = (0.25, 0.5, 0.75)
UNIFORM_EVERY = 5
HUB_ROWS = 7
LONGEST = 256
HUB = -1
SLOT_CYCLE = (1, HUB, 8, 9, HUB, 16, 17, HUB, 7, 2, HUB, 24, 15, HUB, 10, 3, HUB, 23, 1, HUB)

Case = collections.namedtuple("Case", "tag B n C M per parts kernel relu_off position_major")
#        tag          B  n        C    M    per parts
CASES = [
    Case("c64-per3", 2, 24004, 64, 128, 3, 4001, "shfl<64>", True, True),
    Case("c128-per5", 3, 24019, 128, 128, 5, 3603, "shfl<64>, two channel chunks", False, False),
    Case("c32-per6", 2, 95003, 32, 128, 6, 3959, "stream<32>", True, True),
    Case("c16-per6", 3, 110023, 16, 128, 6, 3439, "stream<16>", False, False),
    Case("c8-per4", 2, 200003, 8, 128, 4, 3126, "stream<8>", False, False),
    Case("c32-per16", 2, 262143, 32, 256, 16, 4096, "stream<32>, s_gv full", False, False),
    Case("c32-per17", 2, 262150, 32, 256, 17, 3856, "shfl<32>", False, False),
    Case("c16-per17", 2, 524301, 16, 256, 17, 3856, "shfl<16>", False, False),
    Case("c8-per17", 2, 1048589, 8, 256, 17, 3856, "shfl<8>", False, False),
]
BY_TAG = {c.tag: c for c in CASES}


def plan(B, n, C):
    """(groups, per, parts): lane groups per workgroup, consecutive points per lane group, workgroups (= partial records per
    channel) -- csr_pts_per_group() and csr_partials()"""
    G = B * n
    ct = min(C, 64)
    groups = BS // ct
    per = max(1, -(-G // (WGS * groups)))
    parts = -(-G // (groups * per))
    return groups, per, parts


def kernel(B, n, C, records):
    """which kernel csr_collapse() launches"""
    _, per, _ = plan(B, n, C)
    ct = min(C, 64)
    if not records:
        return f"gather<{ct}>"
    return f"stream<{ct}>" if ct < 64 and per <= STREAM_PMAX else f"shfl<{ct}>"


def windows(B, n, C, b):
    """[(first, end)) local point ranges of cloud b's windows, ascending"""
    groups, per, _ = plan(B, n, C)
    w = WINDOW_GROUPS * per
    n_end = n - (groups * per + 5) if b == B - 1 else n
    out = [(0, w)] + [(int(n * fr) - w // 2, int(n * fr) - w // 2 + w) for fr in FRACTIONS] + [(n_end - w, n_end)]
    assert all(a1 >= e0 for (_, e0), (a1, _) in zip(out, out[1:])) and out[0][0] == 0, "cloud too small for its windows"
    return out


def _wanted(B, n, C, b, rng, rows):
    """{local point: wanted list length, or HUB} over the windows of cloud b"""
    groups, per, _ = plan(B, n, C)
    want, live, slot = {}, set(), 0
    wins = windows(B, n, C, b)
    for a, e in wins:
        first = -(-(b * n + a) // per) * per - b * n  # the lane groups wholly inside the window, by their first local point
        for o, q in enumerate(range(first, e - per + 1, per)):
            if o % 2 == 0 and per >= 3:
                want[q], want[q + 1], want[q + 2] = SLOT_CYCLE[slot % len(SLOT_CYCLE)], 0, SLOT_CYCLE[(slot + 1) % len(SLOT_CYCLE)]
                slot += 2
            else:
                want[q] = HUB
                live.add(q + 1)  # not empty; its length is drawn below
    want[0] = HUB                # the cloud's first point
    want[wins[-1][1] - 1] = HUB  # the last point with edges: the cloud's last one, except in the last cloud
    free = [p for a, e in wins for p in range(a, e) if p not in want]
    placed = sum(v for v in want.values() if v > 0)
    dmax = int(np.clip(4 * (4 * rows - placed) // max(1, len(free)), 2, 24))
    for p in free:
        d = int(dmax * rng.random() ** 3)
        want[p] = max(d, 1) if p in live else d
    hubs = [p for p, v in want.items() if v == HUB]
    need = -(-rows // HUB_ROWS) + 2
    spare = [p for p in free if want[p] <= 2]
    rng.shuffle(spare)
    for p in spare[:max(0, need - len(hubs))]:
        want[p] = HUB
    return want


def build(B, n, C, M, seed):
    """-> idx (B, M, 32) int32 with values in [0, n), dp (B, 3, M, 32) float32 in [-1, 1]"""
    groups, per, _ = plan(B, n, C)
    rng = np.random.default_rng(seed)
    idx = np.empty((B, M, K), dtype=np.int32)
    for b in range(B):
        wins = windows(B, n, C, b)
        outside = np.concatenate([np.arange(e0, a1) for (_, e0), (a1, _) in zip(wins, wins[1:])])  # (nothing behind the end window)
        win_rows = [m for m in range(M) if m % UNIFORM_EVERY]
        want = _wanted(B, n, C, b, rng, len(win_rows))
        hubs = sorted(p for p, v in want.items() if v == HUB)
        assert len(hubs) * HUB_ROWS >= len(win_rows), "too few hubs for the rows"
        left = {p: v for p, v in want.items() if v != HUB and v > 0}  # single edges still to place
        assert sum(left.values()) <= 7 * len(win_rows) and max(left.values()) <= len(win_rows), "more single edges than the rows hold"
        # every hub serves at least one row (a hub is a place that must not be empty), the other rows pick theirs with a skew
        serves = list(hubs) + [hubs[min(int(len(hubs) * rng.random() ** 2), len(hubs) - 1)] for _ in range(len(win_rows) - len(hubs))]
        load = collections.Counter()
        order = rng.permutation(len(win_rows))
        hub_of = {}
        for o, h in zip(order, serves):
            while load[h] >= HUB_ROWS:
                h = hubs[(hubs.index(h) + 1) % len(hubs)]
            load[h] += 1
            hub_of[win_rows[o]] = h
        for m in range(M):
            if m % UNIFORM_EVERY == 0:
                idx[b, m] = outside[rng.integers(0, len(outside), size=K)]
                continue
            r = len(win_rows) - win_rows.index(m)  # rows left, this one included
            total = sum(left.values())
            live = sorted(left, key=lambda p: left[p] + rng.random(), reverse=True)
            k = max(int(rng.integers(0, 8)), total - 7 * (r - 1), sum(1 for p in live if left[p] == r))
            k = min(k, 7, len(live))
            singles = live[:k]
            for p in singles:
                left[p] -= 1
                if not left[p]:
                    del left[p]
            row = [hub_of[m]] + singles
            idx[b, m] = row + [row[0]] * (K - len(row))
        assert not left
    dp = rng.uniform(-1.0, 1.0, size=(B, 3, M, K)).astype(np.float32)
    return idx, dp


def describe(idx, B, n, C):
    """The lists that idx makes, as the lane groups of the collapse see them (numpy, int64):
    deg (G,) list lengths; group_lists (lane groups,) non-empty lists per group; multi: ids of the groups with two or more;
    interior: ids of the groups with an empty list between two non-empty ones; straddle: {boundary b * n: id of the group that
    holds it}; straddle_sides: {boundary: (non-empty lists below it, at or above it) inside that group}; last_wg: first point of
    the last workgroup; lengths: the list lengths among the points of the multi groups; and the point sets the GPU test looks
    at row by row: pts_straddle, pts_interior, pts_last2 (the last two workgroups)."""
    groups, per, parts = plan(B, n, C)
    G = B * n
    flat = idx.reshape(B, -1).astype(np.int64) + (np.arange(B, dtype=np.int64) * n)[:, None]
    deg = np.bincount(flat.ravel(), minlength=G)
    ngroups = -(-G // per)
    padded = np.zeros(ngroups * per, dtype=np.int64)
    padded[:G] = deg
    live = (padded > 0).reshape(ngroups, per)
    group_lists = live.sum(1)
    multi = np.flatnonzero(group_lists >= 2)
    first = np.where(live.any(1), live.argmax(1), per)
    last = np.where(live.any(1), per - 1 - live[:, ::-1].argmax(1), -1)
    span = np.maximum(last - first + 1, 0)
    interior = np.flatnonzero(span > group_lists)  # a hole between the first and the last non-empty list
    straddle, sides = {}, {}
    for b in range(1, B):
        q = (b * n) // per
        straddle[b * n] = q
        cut = b * n - q * per
        sides[b * n] = (int(live[q, :cut].sum()), int(live[q, cut:].sum()))
    last_wg = (parts - 1) * groups * per
    pts = lambda ids: np.concatenate([np.arange(q * per, min((q + 1) * per, G)) for q in ids]) if len(ids) else np.zeros(0, np.int64)
    return {
        "groups": groups, "per": per, "parts": parts, "G": G, "deg": deg, "group_lists": group_lists, "multi": multi,
        "interior": interior, "straddle": straddle, "straddle_sides": sides, "last_wg": last_wg,
        "lengths": np.unique(padded.reshape(ngroups, per)[multi]), "longest": int(deg.max()),
        "pts_straddle": pts(sorted(straddle.values())), "pts_interior": pts(interior),
        "pts_last2": np.arange(max(0, (parts - 2) * groups * per), G),
    }
