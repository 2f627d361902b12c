"""Numpy expectations for the side-path kernels at sizes past 64 stripes, one
scan block and one sort digit (test_gpu_side_scale.py): image builders, whole
streams and closed-form totals, and the rule that names the groups on which the
plain-Python models are run.  test_side_scale_cpu.py checks every builder here
against those models at small sizes.  Nothing here calls the engine."""
from __future__ import annotations

import numpy as np

from helpers import abi, blank_groups, fld, set_fld

# the engine's launch geometry (raft_engine_impl.h) and rocprim's scan blocks of
# eight-byte items: 256 x 8 by default, 256 x 15 in its tuned configuration
HDR_STRIPES = 64
BLOCK = 256
SCAN_BLOCKS = (2048, 3840)
ISO = -2                                 # the isolation word's place in a group's canonical words


def cols(state, R: int, name: str) -> np.ndarray:
    """[G, R] int64: field `name` of every replica."""
    return np.stack([fld(state, R, r, name) for r in range(R)], -1).astype(np.int64)


def waves(G: int, R: int) -> dict:
    """Waves a call over G groups of R launches, per kernel shape."""
    gpw = 64 // R
    return {"tile": -(-G * R // 64), "gpw": -(-G // gpw), "lane": -(-G // 64)}


# ---- the slice rule ----
def holding(replicas, R: int) -> list:
    """The groups that hold the replicas on both sides of each boundary given in replicas."""
    return sorted({b // R for b in replicas} | {-(-b // R) for b in replicas})


def boundaries(kind: str, R: int) -> list:
    """The group numbers (relative to the call's g0) at which a kernel of this
    shape starts a new workgroup of 4 waves and wraps its 64 stripes."""
    gpw = 64 // R
    if kind == "lane":                                      # one lane per group
        return [BLOCK, 64 * HDR_STRIPES]
    if kind == "gpw":                                       # a wave holds 64 / R whole groups
        return [gpw * 4, gpw * HDR_STRIPES]
    if kind == "tile":                                      # a wave owns 64 consecutive replicas
        return holding((BLOCK, 64 * HDR_STRIPES), R)
    if kind == "scan":                                      # one scan item per replica
        return holding(SCAN_BLOCKS, R)
    raise ValueError(kind)


def slice_groups(n: int, kind: str, R: int, seed: int, g0: int = 0, extra: int = 16) -> np.ndarray:
    """Absolute groups of the range [g0, g0 + n) the Python models are run on:
    the first and the last, two on each side of every boundary of `kind`
    (relative to g0, where the kernel counts its waves from), and `extra` from
    default_rng(seed).  Sorted, unique, all inside the range."""
    rel = {0, n - 1}
    for b in boundaries(kind, R):
        rel.update((b - 2, b - 1, b, b + 1))
    rel.update(np.random.default_rng(seed).choice(n, min(extra, n), replace=False).tolist())
    return g0 + np.array(sorted(x for x in rel if 0 <= x < n), dtype=np.int64)


def complement(n: int, sel) -> np.ndarray:
    """Boolean [n]: True outside the selection `sel` of indices."""
    m = np.ones(n, bool)
    m[np.asarray(sel, dtype=np.int64)] = False
    return m


# ---- drain and machine: committed runs of (g + k) % 7 entries ----
def run_lengths(G: int, R: int) -> np.ndarray:
    return (np.arange(G)[:, None] + np.arange(R)[None, :]) % 7


def committed_image(G: int, R: int, cap: int, seed: int = 7):
    """(state, terms, cmds, lens): replica k of group g holds, and has
    committed, (g + k) % 7 entries of random terms and commands."""
    w = blank_groups(G, R)
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 9, (G, R, cap), dtype=np.int32)
    c = rng.integers(0, 2 ** 32, (G, R, cap), dtype=np.uint32)
    lens = run_lengths(G, R)
    for k in range(R):
        for name in ("last", "phys", "commit"):
            set_fld(w, R, k, name, lens[:, k])
        set_fld(w, R, k, "term", 9)
    return w, t, c, lens


def drain_stream(terms, cmds, lo, hi, g0: int = 0, n=None, replica: int = -1) -> np.ndarray:
    """Every entry [lo, hi) of each selected replica (lo, hi: [G, R]) in
    (group, replica, index) order, as abi.APPLIED_DTYPE records."""
    G, R = lo.shape
    n = G - g0 if n is None else n
    rs = np.arange(R) if replica < 0 else np.array([replica])
    lo, hi = lo[g0:g0 + n][:, rs].astype(np.int64), hi[g0:g0 + n][:, rs].astype(np.int64)
    cnt = np.maximum(hi - lo, 0).ravel()
    g = np.repeat(np.repeat(np.arange(g0, g0 + n), len(rs)), cnt)
    r = np.repeat(np.tile(rs, n), cnt)
    first = np.cumsum(cnt) - cnt
    i = np.arange(cnt.sum()) - np.repeat(first, cnt) + np.repeat(lo.ravel(), cnt)
    out = np.zeros(len(g), abi.APPLIED_DTYPE)
    out["group"], out["replica"], out["index"] = g, r, i
    out["term"], out["cmd"] = terms[g, r, i], cmds[g, r, i]
    return out


def stripe_total(per_wave, drop: int | None = None) -> int:
    """A striped total as DevWords::fetch sums it: wave w adds per_wave[w] to
    line w mod HDR_STRIPES, the lines are summed.  drop: a line that is lost."""
    lines = np.zeros(HDR_STRIPES, np.int64)
    np.add.at(lines, np.arange(len(per_wave)) % HDR_STRIPES, np.asarray(per_wave, dtype=np.int64))
    if drop is not None:
        lines[drop] = 0
    return int(lines.sum())


def per_wave(values, width: int) -> np.ndarray:
    """Sums of consecutive runs of `width` items (the last one ragged)."""
    v = np.asarray(values, dtype=np.int64).ravel()
    pad = -len(v) % width
    return np.concatenate([v, np.zeros(pad, np.int64)]).reshape(-1, width).sum(1)


def apply_total(lens, applied, g0: int = 0, n=None) -> int:
    """info["applied"] of an sm_apply on a flat log with no regressed replica."""
    n = lens.shape[0] - g0 if n is None else n
    return int(np.maximum(lens[g0:g0 + n] - applied[g0:g0 + n], 0).sum())


# ---- the machine's reads ----
def lowest_leader(state, R: int) -> np.ndarray:
    """[G]: the lowest replica index with role LEADER, -1 if none."""
    lead = cols(state, R, "role") == abi.LEADER
    return np.where(lead.any(1), lead.argmax(1), -1)


def newest_leader(state, R: int) -> np.ndarray:
    """[G]: the LEADER with the highest currentTerm, the lowest index among equals; -1 if none."""
    lead = cols(state, R, "role") == abi.LEADER
    term = np.where(lead, cols(state, R, "term"), -1)
    return np.where(lead.any(1), term.argmax(1), -1)


def sm_get_expect(state, heads, regs, R: int, groups, keys, replicas) -> np.ndarray:
    groups, keys = np.asarray(groups, dtype=np.int64), np.asarray(keys, dtype=np.uint32)
    r = np.broadcast_to(np.asarray(replicas, dtype=np.int64), groups.shape)
    r = np.where(r < 0, lowest_leader(state, R)[groups], r)
    ok = r >= 0
    rc = np.where(ok, r, 0)
    S = regs.shape[2]
    out = np.zeros(len(groups), abi.SM_VALUE_DTYPE)
    out["value"] = np.where(ok, regs[groups, rc, keys & np.uint32(S - 1)], 0)
    out["replica"] = np.where(ok, r, -1)
    out["applied"] = np.where(ok, heads["applied"][groups, rc], 0)
    out["commit"] = np.where(ok, cols(state, R, "commit")[groups, rc], 0)
    return out


def sm_check_expect(heads) -> np.ndarray:
    R = heads.shape[1]
    bad = np.zeros(heads.shape[0], bool)
    for a in range(R):
        for b in range(a + 1, R):
            bad |= (heads["lost"][:, a] == 0) & (heads["lost"][:, b] == 0) & \
                (heads["applied"][:, a] == heads["applied"][:, b]) & (heads["hash"][:, a] != heads["hash"][:, b])
    return bad.astype(np.uint8)


# ---- a mix of roles: leaders, sessions, committed prefixes ----
def led_image(G: int, R: int, cap: int, seed: int = 21, leaderless: int = 11):
    """(state, terms, cmds): every replica holds 1 to cap - 2 entries with a
    committed prefix, random next / match sessions and armed timers; replica
    g % R leads group g in term 5 + g % 3, every 13th group has a deposed
    second leader of term 2, and every `leaderless`-th group has no leader.
    The leader's last entry is of its own term in the groups with g % 4 == 1.
    Every 17th group carries a running isolation of replica g % R."""
    rng = np.random.default_rng(seed)
    w = blank_groups(G, R)
    gi = np.arange(G)
    t = rng.integers(1, 5, (G, R, cap), dtype=np.int32)
    c = rng.integers(1, 2 ** 32, (G, R, cap), dtype=np.uint32)
    for r in range(R):
        last = rng.integers(1, cap - 1, G)
        set_fld(w, R, r, "last", last)
        set_fld(w, R, r, "phys", last)
        set_fld(w, R, r, "commit", rng.integers(0, cap - 1, G) % (last + 1))
        set_fld(w, R, r, "term", 5 + gi % 3)
        set_fld(w, R, r, "voted", gi % R)
        set_fld(w, R, r, "flags", abi.FL_ARMED)
        set_fld(w, R, r, "election_ms", 5000 + rng.integers(0, 5000, G))
        lead = (gi % R == r) & (gi % leaderless != 0)
        old = ((gi + 2) % R == r) & (gi % 13 == 0)
        role = np.where(lead | old, abi.LEADER, abi.FOLLOWER)
        set_fld(w, R, r, "role", role)
        set_fld(w, R, r, "term", np.where(old & ~lead, 2, 5 + gi % 3))
        set_fld(w, R, r, "flags", np.where(lead | old, abi.FL_HB_ACTIVE, abi.FL_ARMED))
        own = np.flatnonzero(lead & (gi % 4 == 1))
        t[own, r, last[own] - 1] = 5 + own % 3
    nf = R * abi.NUM_FIELDS
    w[:, nf:nf + 2 * R * R] = rng.integers(0, cap, (G, 2 * R * R))
    w[:, ISO] = np.where(gi % 17 == 0, 6 << 8 | gi % R, 0)
    return w, t, c


# ---- restart ----
def restart_totals(state, sel, R: int, amnesia: bool) -> dict:
    """raft_restart_info of restarting the replicas sel [n, R] of `state` [n, words]."""
    role, last = cols(state, R, "role"), cols(state, R, "last")
    return {"restarted": int(sel.sum()), "leaders": int((sel & (role == abi.LEADER)).sum()),
            "entries_dropped": int(last[sel].sum()) if amnesia else 0}


def sparse_mask(n: int, R: int, seed: int, one_in: int = 50) -> np.ndarray:
    """n mask bytes with about one replica in `one_in` set, a few groups with
    every replica (several per wave) and bits at or above R set here and there
    (ignored by the kernel)."""
    rng = np.random.default_rng(seed)
    sel = rng.random((n, R)) < 1.0 / one_in
    sel[::997] = True
    m = (sel.astype(np.uint8) << np.arange(R, dtype=np.uint8)[None, :]).sum(1).astype(np.uint8)
    if R < 8:
        m[::5] |= np.uint8(1 << R)
    return m


# ---- isolate, heal, list ----
def running(words) -> np.ndarray:
    return (np.asarray(words, dtype=np.int64) >> 8) > 0


def heal_totals(words, mask=None) -> dict:
    """raft_heal_info over the isolation words of the range (mask: its bytes)."""
    words = np.asarray(words, dtype=np.int64)
    run = running(words)
    hit = run if mask is None else run & (((np.asarray(mask, dtype=np.int64) >> (words & 0xFF)) & 1) == 1)
    return {"healed": int(hit.sum()), "idle": int((~run).sum()), "kept": int((run & ~hit).sum())}


def isolated_expect(state, R: int, g0: int = 0, n=None, max_events=None):
    """raft_engine_list_isolated of groups [g0, g0 + n): (info, records)."""
    n = state.shape[0] - g0 if n is None else n
    words = state[g0:g0 + n, ISO].astype(np.int64)
    at = np.flatnonzero(running(words))
    rep = words[at] & 0xFF
    role = cols(state[g0:g0 + n], R, "role")
    out = np.zeros(len(at), abi.ISOLATED_DTYPE)
    out["group"], out["replica"], out["remaining"] = g0 + at, rep, words[at] >> 8
    out["role"] = np.where(rep < R, role[at, np.minimum(rep, R - 1)], -1)
    room = len(at) if max_events is None else min(int(max_events), len(at))
    return dict(delivered=room, pending=len(at) - room, running=len(at)), out[:room]


# ---- no-op entries ----
def noop_totals(state, terms, R: int, cap: int, textbook: bool, g0: int = 0, n=None) -> dict:
    """raft_noop_info of an append over groups [g0, g0 + n) of a flat log."""
    n = state.shape[0] - g0 if n is None else n
    st, tm = state[g0:g0 + n], terms[g0:g0 + n]
    L = newest_leader(st, R)
    ok = L >= 0
    Lc = np.where(ok, L, 0)
    at = np.arange(n)
    T, last, phys = (cols(st, R, f)[at, Lc] for f in ("term", "last", "phys"))
    lt = np.where(last >= 1, tm[at, Lc, np.clip(last - 1, 0, cap - 1)], 0)
    cur = ok & (last >= 1) & (lt == T)
    todo = ok & ~cur
    full = todo & ((last >= cap) if textbook else (phys >= cap))
    ghost = todo & ~full & (phys != last) & (not textbook)
    return {"appended": int((todo & ~full).sum()), "current": int(cur.sum()), "no_leader": int((~ok).sum()),
            "log_full": int(full.sum()), "ghosted": int(ghost.sum())}


# ---- reads, transfers, installs: a settled image with known exceptions ----
def settled_image(G: int, R: int, cap: int):
    """(state, terms, cmds): replica g % R leads group g in term 3 (none in
    every 11th group); every replica holds and has committed 4 entries, the
    last of term 3 (of term 2 in every 5th group: nothing of the leader's term
    is committed there); followers are idle and armed.  The exceptions, on
    followers: replica (g + 1) % R of every third group lags with one entry;
    replica (g + 2) % R is in term 9 where g % 10 == 3 and electing where
    g % 7 == 3; replica (g + 1) % R is isolated where g % 13 == 4."""
    gi = np.arange(G)
    w = blank_groups(G, R)
    t = np.zeros((G, R, cap), np.int32)
    c = np.random.default_rng(G + R).integers(1, 2 ** 32, (G, R, cap), dtype=np.uint32)
    c[:, 1:] = c[:, :1]                                                # one log in every replica
    t[:, :, :4] = (1, 1, 2, 3)
    t[gi % 5 == 0, :, 3] = 2
    for r in range(R):
        lead = (gi % R == r) & (gi % 11 != 0)
        lag = ((gi + 1) % R == r) & (gi % 3 == 0)
        n = np.where(lag, 1, 4)
        set_fld(w, R, r, "last", n)
        set_fld(w, R, r, "phys", n)
        set_fld(w, R, r, "commit", n)
        set_fld(w, R, r, "term", np.where(((gi + 2) % R == r) & (gi % 10 == 3) & ~lead, 9, 3))
        set_fld(w, R, r, "voted", gi % R + 1)
        set_fld(w, R, r, "role", np.where(lead, abi.LEADER, abi.FOLLOWER))
        busy = ((gi + 2) % R == r) & (gi % 7 == 3) & ~lead
        set_fld(w, R, r, "flags", np.where(lead, abi.FL_HB_ACTIVE, np.where(busy, abi.FL_ARMED | abi.FL_ELECTING, abi.FL_ARMED)))
        set_fld(w, R, r, "election_ms", np.where(lead, 0, 20000 + r))
    w[:, ISO] = np.where(gi % 13 == 4, 5 << 8 | (gi + 1) % R, 0)
    return w, t, c


def last_term_of(state, terms, R: int) -> np.ndarray:
    """[G, R]: the term of each replica's last entry, 0 for an empty log."""
    last = cols(state, R, "last")
    at = np.arange(state.shape[0])[:, None]
    return np.where(last >= 1, terms[at, np.arange(R)[None, :], np.maximum(last - 1, 0)], 0).astype(np.int32)


def evacuate_totals(state, lt, mask, R: int, g0: int = 0, per_group: bool = False) -> dict:
    """raft_evacuate_info of groups [g0, g0 + len(mask)): a candidate is a
    replica outside the mask other than the newest leader; it is behind, else
    busy (or cut off), else it can take over."""
    n = len(mask)
    st, lt = state[g0:g0 + n], lt[g0:g0 + n]
    mk = np.asarray(mask, dtype=np.int64) & ((1 << R) - 1)
    L = newest_leader(st, R)
    Lc = np.where(L >= 0, L, 0)
    at = np.arange(n)
    led = (L >= 0) & (((mk >> Lc) & 1) == 1)
    rs = np.arange(R)[None, :]
    cand = (rs != Lc[:, None]) & (((mk[:, None] >> rs) & 1) == 0)
    last, role, fl = cols(st, R, "last"), cols(st, R, "role"), cols(st, R, "flags")
    behind = (last != last[at, Lc][:, None]) | (lt != lt[at, Lc][:, None])
    words = st[:, ISO].astype(np.int64)
    cut = np.where(running(words), words & 0xFF, -1)
    busy = (role != abi.FOLLOWER) | ((fl & abi.FL_ARMED) == 0) | \
        ((fl & (abi.FL_ELECTING | abi.FL_BACKOFF | abi.FL_PENDING_RST)) != 0) | (rs == cut[:, None])
    sent = led & (cand & ~behind & ~busy).any(1)
    none = led & ~sent
    each = {"led": led, "sent": sent, "no_target": none, "behind": none & (cand & behind).any(1),
            "busy": none & (cand & ~behind & busy).any(1)}
    return each if per_group else {k: int(v.sum()) for k, v in each.items()}


def install_totals(state, heads, sel, R: int, W: int = 0, per_group: bool = False) -> dict:
    """raft_install_info of installing the eligible replicas sel [n, R] of
    `state` [n, words] with min_lag 0: every eligible replica but the leader
    whose term is not above the leader's is installed."""
    n = state.shape[0]
    L = newest_leader(state, R)
    Lc = np.where(L >= 0, L, 0)
    at = np.arange(n)
    gap = (L >= 0) & (heads["lost"][at, Lc] != 0)
    ok = (L >= 0) & ~gap
    term, phys = cols(state, R, "term"), cols(state, R, "phys")
    other = sel & (np.arange(R)[None, :] != Lc[:, None]) & ok[:, None]
    ahead = other & (term > term[at, Lc][:, None])
    inst = other & ~ahead
    physL = phys[at, Lc]
    kept = physL - (np.maximum(0, physL - W) if W else 0)
    each = {"installed": inst.sum(1), "slots_copied": inst.sum(1) * kept, "no_leader": L < 0, "leader_gapped": gap,
            "ahead": ahead.sum(1)}
    return each if per_group else {k: int(v.sum()) for k, v in each.items()}


def evacuate_mask(n: int, R: int, g0: int, seed: int) -> np.ndarray:
    """n mask bytes over settled_image: random bits, and in half the groups
    every replica but one of the followers with exceptions (g + 1, g + 2)."""
    g = g0 + np.arange(n)
    m = np.random.default_rng(seed).integers(0, 1 << R, n).astype(np.int64)
    full = (1 << R) - 1
    m = np.where(g % 4 == 0, full & ~(1 << (g + 1) % R), np.where(g % 4 == 1, full & ~(1 << (g + 2) % R), m))
    return m.astype(np.uint8)


# ---- the outbox: one scenario for the oracle's Host (outbox_model) and the engine ----
def outbox_kw(G: int, R: int = 5) -> dict:
    """Textbook mode, message drops, no commands of the harness's own: every entry is a proposal."""
    return dict(R=R, G=G, seed=11, log_cap=32, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, drop_ppm=50_000, cmd_ppm=0)


def outbox_scenario(x, n: int, seed: int, warm: int = 40) -> list:
    """On `x` (outbox_model.Host or a RaftEngine): `warm` steps, a submit of n
    records over random groups, a pump (every record is new: proposed), 10 steps,
    a pump cut in the middle of its done stream, a pump without a cut.  Returns
    per pump (info, done, return code, the queue left)."""
    rng = np.random.default_rng(seed)
    groups = rng.integers(0, x.G, n, dtype=np.int64)
    groups[:2] = (0, x.G - 1)
    cmds = (1_000_000 + np.arange(n)).astype(np.uint32)
    x.step(warm)
    x.outbox_configure(n + 8, 0)
    x.outbox_submit(groups, cmds, cmds.astype(np.int64))
    out = []
    for cut in (None, "half", None):
        if cut == "half":
            x.step(10)
            cut = max(1, out[0][0]["accepted"] // 3)                    # (an accepted proposal commits in these steps, mostly)
        info, done = x.outbox_pump(cut)
        out.append((info, done, x.last_status, x.outbox_read()))
    return out


def outbox_closed(points, n: int) -> None:
    """What the three infos must say whatever the verdicts were."""
    (a, da, _, qa), (b, db, _, qb), (c, dc, _, qc) = points
    assert a["queued"] == a["retried"] == a["left"] == n and len(da) == 0 and len(qa) == n
    assert a["accepted"] + a["ghosted"] + a["no_leader"] + a["log_full"] == n
    assert b["queued"] == n and len(db) == b["committed"] + b["expired"] and b["left"] == n - len(db) == len(qb)
    fin = len(db) + b["deferred"]
    assert b["pending"] + b["orphaned"] + b["unknown"] + b["retried"] + fin == n
    assert c["queued"] == len(qb) and len(dc) == c["committed"] >= b["deferred"] and c["deferred"] == 0
    assert c["left"] == len(qb) - len(dc) == len(qc)
    for info, done in ((b, db), (c, dc)):
        assert sum(info["age_hist"]) == info["committed"] and np.all(done["status"] == abi.OUTBOX_COMMITTED)


# ---- replay after a poll: the WAL test's image, with full rows here and there ----
def wal_image(G: int, R: int, cap: int, full_every: int = 500):
    """(state, terms, cmds, lens): replica k of group g is in term 9 + g % 3,
    voted for k, and holds (g + k) % 7 entries -- all `cap` in every
    `full_every`-th group.  Nothing is committed."""
    gi = np.arange(G)
    lens = np.where((gi % full_every == 0)[:, None], cap, run_lengths(G, R))
    w = blank_groups(G, R)
    j = np.arange(cap, dtype=np.int64)[None, None, :]
    key = gi[:, None, None] * 131 + np.arange(R)[None, :, None] * 7 + j
    t = (1 + key % 8).astype(np.int32)
    c = ((key * 2654435761) & 0xFFFFFFFF).astype(np.uint32)
    for k in range(R):
        set_fld(w, R, k, "last", lens[:, k])
        set_fld(w, R, k, "phys", lens[:, k])
        set_fld(w, R, k, "term", 9 + gi % 3)
        set_fld(w, R, k, "voted", k)
    return w, t, c, lens


def wal_stream(state, terms, cmds, lens, R: int) -> np.ndarray:
    """A fresh cursor's poll of wal_image: per replica a HARDSTATE, then its entries."""
    G = state.shape[0]
    cnt = (lens + 1).ravel().astype(np.int64)
    g = np.repeat(np.repeat(np.arange(G), R), cnt)
    r = np.repeat(np.tile(np.arange(R), G), cnt)
    pos = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)   # 0: the HARDSTATE, then entry pos - 1
    hs = pos == 0
    i = np.maximum(pos - 1, 0)
    out = np.zeros(len(g), abi.WAL_RECORD_DTYPE)
    names = out.dtype.names                                             # group, replica, kind, index, term, cmd, aux
    out[names[0]], out[names[1]] = g, r
    out[names[2]] = np.where(hs, abi.WAL_HARDSTATE, abi.WAL_ENTRY)
    out[names[3]] = np.where(hs, -1, i)
    out[names[4]] = np.where(hs, cols(state, R, "term")[g, r], terms[g, r, i])
    out[names[5]] = np.where(hs, 0, cmds[g, r, i])
    out[names[6]] = np.where(hs, cols(state, R, "voted")[g, r], 0)
    return out
