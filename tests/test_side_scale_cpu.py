"""The numpy expectations of tests/side_scale_model.py against the plain-Python
models, over the whole range at G = 203 and G = 1,000, and the slice rule's
promises: a wrong expectation is found here, without a GPU.  The last test
shows why the GPU tests run at 20,011 groups: a striped total that loses one
of its 64 lines is still right at G = 203."""
import numpy as np
import pytest

import apply_model as AM
import client_model as CM
import nemesis_model as NM
import noop_model as NO
import oracle as O
import read_model as RD
import restart_model as RM
import side_scale_model as S
import outbox_model as OM
import replay_model as RP
import sm_model as SM
import wal_model as WM
import snapshot_model as SN
import transfer_model as TM
from helpers import abi

SIZES = [203, 1_000]
R, CAP = 5, 16


@pytest.mark.parametrize("G", SIZES)
def test_drain_stream_is_the_models(G):
    w, t, c, lens = S.committed_image(G, R, CAP)
    zero = np.zeros((G, R), np.int64)
    for g0, n, q in ((0, G, -1), (0, G, 2), (G // 5 + 1, G // 2 + 3, -1), (7, 64, 4)):
        want, info = AM.drain(w, t, c, zero.copy(), R, CAP, g0=g0, n=n, replica=q)
        got = S.drain_stream(t, c, zero, lens, g0, n, q)
        assert got.dtype == want.dtype and np.array_equal(got, want), (g0, n, q)
        assert info["delivered"] == len(got) and info["regressed"] == 0
    part = np.minimum(lens, 2)                                        # a cursor in the middle of every run
    want, _ = AM.drain(w, t, c, part.copy(), R, CAP)
    assert np.array_equal(S.drain_stream(t, c, part, lens), want)


@pytest.mark.parametrize("Rr", [5, 3])
@pytest.mark.parametrize("G", SIZES)
def test_machine_expectations_are_the_models(G, Rr):
    w, t, c, lens = S.committed_image(G, Rr, CAP)
    mach = SM.Machine(G, Rr, 8)
    g0, n = G // 5 + 1, G // 2 + 3
    info = SM.apply(w, t, c, mach, Rr, CAP, g0=g0, n=n)
    assert info["applied"] == S.apply_total(lens, np.zeros_like(lens), g0, n) and info["regressed"] == 0
    before = mach.applied.copy()
    info = SM.apply(w, t, c, mach, Rr, CAP)
    assert info["applied"] == S.apply_total(lens, before) and np.array_equal(mach.applied, lens)
    heads = mach.heads()
    bad = np.arange(0, G, 97)
    heads["hash"][bad, 1] ^= np.uint64(1)                             # replicas 1 and 1 + 7 k share a length...
    heads["applied"][bad, 0] = heads["applied"][bad, 1]               # ...and now replica 0 does too
    m2 = mach.copy()
    m2.hash, m2.applied = heads["hash"].copy(), heads["applied"].astype(np.int64)
    assert np.array_equal(S.sm_check_expect(heads), SM.check(m2)) and S.sm_check_expect(heads)[bad].all()
    st, _, _ = S.led_image(G, Rr, CAP)
    rng = np.random.default_rng(3)
    groups = rng.integers(0, G, 3 * G)
    keys = rng.integers(0, 2 ** 32, 3 * G, dtype=np.uint32)
    reps = rng.integers(-1, Rr, 3 * G)
    got = S.sm_get_expect(st, heads, mach.reg, Rr, groups, keys, reps)
    want = SM.get(st, m2, Rr, groups.tolist(), keys.tolist(), reps.tolist())
    assert np.array_equal(got, want) and (got["replica"] == -1).any() and got["value"].any()


@pytest.mark.parametrize("G", SIZES)
def test_leader_columns_are_the_models(G):
    st, _, _ = S.led_image(G, R, CAP)
    low, new = S.lowest_leader(st, R), S.newest_leader(st, R)
    assert np.array_equal(low, CM.leaders(st, R)["leader"])
    assert np.array_equal(low, [SM.leader_of(st, R, g) for g in range(G)])
    assert np.array_equal(new, [RD.newest_leader(st, R, g) for g in range(G)])
    assert (low != new).any() and (low < 0).any() and (CM.leaders(st, R)["n_leaders"] == 2).any()


@pytest.mark.parametrize("amnesia", [False, True])
@pytest.mark.parametrize("G", SIZES)
def test_restart_totals_are_the_models(G, amnesia):
    st, _, _ = S.led_image(G, R, CAP)
    g0, n = G // 5 + 1, G // 2 + 3
    mask = S.sparse_mask(n, R, seed=4, one_in=10)
    sel = RM.select_mask(mask, R)
    want = S.restart_totals(st[g0:g0 + n], sel, R, amnesia)
    info = RM.restart(st[g0:g0 + n].copy(), sel, R=R, seed=1, step=0, gid0=g0, emin=5000, emax=10000,
                      flags=RM.AMNESIA if amnesia else 0)
    assert info == want and want["leaders"] > 0 and want["restarted"] > n * R // 20
    assert (want["entries_dropped"] > 0) == amnesia


@pytest.mark.parametrize("G", SIZES)
def test_nemesis_expectations_are_the_models(G):
    st, _, _ = S.led_image(G, R, CAP)
    st[5, S.ISO] = 3                                                  # expired: not running
    st[6, S.ISO] = 9 << 8 | R                                         # a replica index the group does not have
    for g0, n, cut in ((0, G, None), (G // 5 + 1, G // 2 + 3, 4), (0, G, 0)):
        info, rec = S.isolated_expect(st, R, g0, n, cut)
        winfo, wrec = NM.list_isolated(st, R, g0, n, cut)
        assert info == winfo and np.array_equal(rec, wrec.astype(abi.ISOLATED_DTYPE)), (g0, n, cut)
    g0, n = G // 5 + 1, G // 2 + 3
    mask = np.random.default_rng(6).integers(0, 32, n).astype(np.uint8)
    assert S.heal_totals(st[g0:g0 + n, S.ISO], mask) == NM.heal(st.copy(), R, mask, g0)
    assert S.heal_totals(st[:, S.ISO]) == NM.heal(st.copy(), R)
    t = S.heal_totals(st[g0:g0 + n, S.ISO], mask)
    assert t["healed"] > 0 and t["kept"] > 0 and t["idle"] > 0


@pytest.mark.parametrize("textbook", [False, True], ids=["reference", "textbook"])
@pytest.mark.parametrize("G", SIZES)
def test_noop_totals_are_the_models(G, textbook):
    st, t, c = S.led_image(G, R, CAP)
    kw = dict(R=R, G=G, log_cap=CAP, mode=abi.MODE_TEXTBOOK if textbook else abi.MODE_REFERENCE)
    o = O.Oracle(abi.make_params(**kw))
    o.write_state(st)
    o.write_log(t, c)
    g0, n = G // 5 + 1, G // 2 + 3
    want = S.noop_totals(st, t, R, CAP, textbook, g0, n)
    info, _, _, _ = NO.append_noops(o, g0, n, 7, textbook)
    assert info == want and want["appended"] > 0 and want["current"] > 0 and want["no_leader"] > 0
    st2, (t2, _) = o.read_state(), o.read_log()
    again = S.noop_totals(st2, t2, R, CAP, textbook, g0, n)            # a second call appends nothing
    assert again["appended"] == 0 and again["current"] == want["current"] + want["appended"]
    o.close()


@pytest.mark.parametrize("kind", ["lane", "gpw", "tile", "scan"])
@pytest.mark.parametrize("Rr", [5, 3])
def test_slice_rule_keeps_its_promises(kind, Rr):
    for n, g0 in ((20_011, 0), (12_345, 4_099), (203, 0), (3, 1)):
        s = S.slice_groups(n, kind, Rr, seed=1, g0=g0)
        assert s.min() >= g0 and s.max() < g0 + n and np.all(np.diff(s) > 0)
        assert g0 in s and g0 + n - 1 in s
        for b in S.boundaries(kind, Rr):
            for x in (b - 2, b - 1, b, b + 1):
                assert (g0 + x in s) == (0 <= x < n), (kind, n, b, x)
        assert len(s) >= min(n, 16)
        assert np.array_equal(s, S.slice_groups(n, kind, Rr, seed=1, g0=g0))       # the seed fixes it
    gpw = 64 // Rr
    assert S.boundaries("gpw", Rr) == [gpw * 4, gpw * 64] and S.boundaries("lane", Rr) == [256, 4096]
    held = S.slice_groups(20_011, "scan", Rr, seed=1)                   # the groups holding the items beside a block's end
    for item in (2047, 2048, 3839, 3840):
        assert item // Rr in held and item // Rr - 1 in held and item // Rr + 1 in held
    held = S.slice_groups(20_011, "tile", Rr, seed=1)                   # ... and the replicas beside a tile kernel's
    for rep in (255, 256, 4095, 4096):                                  # workgroup and its stripe wrap
        assert rep // Rr in held and rep // Rr - 1 in held and rep // Rr + 1 in held
    assert not S.complement(10, [0, 9])[[0, 9]].any() and S.complement(10, [0, 9]).sum() == 8


def test_a_lost_stripe_shows_at_20011_groups_and_not_at_203():
    """Every closed-form total of the GPU tests, summed as the kernels sum it
    (one contribution per wave, folded mod 64 lines), with line 63 lost: at
    G = 203 no wave reaches line 63 and the total is still right; at G = 20,011
    every line is used several times over and every total is wrong."""
    for G, seen in ((203, False), (20_011, True)):
        wv = S.waves(G, R)
        assert (min(wv.values()) > S.HDR_STRIPES) == seen
        _, _, _, lens = S.committed_image(G, R, 8)
        st, t, _ = S.led_image(G, R, CAP)
        sel = RM.select_mask(S.sparse_mask(G, R, seed=4), R)
        role = S.cols(st, R, "role")
        gpw = 64 // R
        run = S.running(st[:, S.ISO])
        todo = (S.newest_leader(st, R) >= 0)
        totals = {
            "sm applied": (S.per_wave(lens, 64), S.apply_total(lens, np.zeros_like(lens))),
            "restarted": (S.per_wave(sel.sum(1), gpw), S.restart_totals(st, sel, R, False)["restarted"]),
            "restart leaders": (S.per_wave((sel & (role == abi.LEADER)).sum(1), gpw),
                                S.restart_totals(st, sel, R, False)["leaders"]),
            "entries dropped": (S.per_wave((S.cols(st, R, "last") * sel).sum(1), gpw),
                                S.restart_totals(st, sel, R, True)["entries_dropped"]),
            "healed": (S.per_wave(run, 64), S.heal_totals(st[:, S.ISO])["healed"]),
            "idle": (S.per_wave(~run, 64), S.heal_totals(st[:, S.ISO])["idle"]),
            "noop led": (S.per_wave(todo, 64), G - S.noop_totals(st, t, R, CAP, True)["no_leader"]),
        }
        sw, stt, _ = S.settled_image(G, R, CAP)
        lt = S.last_term_of(sw, stt, R)
        mask = S.evacuate_mask(G, R, 0, 8)
        for k, v in S.evacuate_totals(sw, lt, mask, R, per_group=True).items():
            totals[f"evacuate {k}"] = (S.per_wave(v, 64), S.evacuate_totals(sw, lt, mask, R)[k])
        heads = np.zeros((G, R), abi.SM_HEAD_DTYPE)
        heads["lost"][::29] = 1
        isel = RM.select_mask(np.random.default_rng(9).integers(0, 1 << R, G).astype(np.uint8), R)
        for k, v in S.install_totals(sw, heads, isel, R, per_group=True).items():
            totals[f"install {k}"] = (S.per_wave(v, gpw), S.install_totals(sw, heads, isel, R)[k])
        for name, (contrib, whole) in totals.items():
            assert S.stripe_total(contrib) == whole, (G, name)
            assert (S.stripe_total(contrib, drop=63) != whole) == seen, (G, name)


@pytest.mark.parametrize("Rr", [5, 3])
@pytest.mark.parametrize("G", SIZES)
def test_settled_image_totals_are_the_models(G, Rr):
    st, t, c = S.settled_image(G, Rr, CAP)
    lt = S.last_term_of(st, t, Rr)
    assert np.array_equal(lt, TM.last_terms(st, t, Rr))
    g0, n = G // 5 + 1, G // 2 + 3
    mask = S.evacuate_mask(n, Rr, g0, 8)
    want = TM.evacuate(st.copy(), mask, Rr, g0, lt)
    assert S.evacuate_totals(st, lt, mask, Rr, g0) == want and want["sent"] > 0 and want["no_target"] > 0
    assert want["behind"] > 0 and want["busy"] > 0
    heads = np.zeros((G, Rr), abi.SM_HEAD_DTYPE)
    heads["applied"] = S.cols(st, Rr, "commit")
    heads["lost"][::29] = 1
    sel = RM.select_mask(np.random.default_rng(9).integers(0, 1 << Rr, n).astype(np.uint8), Rr)
    for W in (0, 16):
        info = SN.install(st[g0:g0 + n].copy(), t[g0:g0 + n].copy(), c[g0:g0 + n].copy(), heads[g0:g0 + n].copy(),
                          np.zeros((n, Rr, 8), np.uint32), sel, R=Rr, cap=CAP, W=W, seed=1, step=0, gid0=g0,
                          emin=5000, emax=10000)
        assert info == S.install_totals(st[g0:g0 + n], heads[g0:g0 + n], sel, Rr, W), W
        assert all(info[k] > 0 for k in SN.INFO_KEYS), info


@pytest.mark.parametrize("G", SIZES)
def test_outbox_scenario_reaches_every_class(G):
    """The scenario of the GPU test on the oracle's Host: the infos keep the
    closed-form relations, and committed, retried and kept records all occur."""
    h = OM.Host(**S.outbox_kw(G))
    pts = S.outbox_scenario(h, G + 3, seed=G)
    h.close()
    S.outbox_closed(pts, G + 3)
    (a, _, _, _), (b, db, _, qb), (c, dc, _, qc) = pts
    assert a["accepted"] > 0 and a["no_leader"] > 0
    assert len(db) > 0 and b["deferred"] > 0 and b["retried"] > 0 and len(qc) > 0
    assert len(np.intersect1d(db["tag"], dc["tag"])) == 0 and np.all(np.diff(db["tag"]) > 0)


@pytest.mark.parametrize("G", SIZES)
def test_wal_stream_is_the_models_and_replays_to_the_source(G):
    cap = 20
    w, t, c, lens = S.wal_image(G, R, cap, full_every=50)
    rec = S.wal_stream(w, t, c, lens, R)
    want, info = WM.poll(w, t, c, WM.fresh(G, R), R, cap)
    assert rec.dtype == want.dtype and np.array_equal(rec, want)
    assert len(rec) == G * R + int(lens.sum()) and info["truncates"] == 0
    st, tt, tc = blank_state(G), np.zeros_like(t), np.zeros_like(c)
    info = RP.replay(st, tt, tc, rec, R=R, cap=cap, seed=1, step=0, emin=5000, emax=10000)
    assert info["malformed"] == 0 and info["applied"] == len(rec) and info["replicas"] == G * R
    assert not RP.persistent_errors(st, tt, tc, w, t, c, R, cap)
    bad = rec.copy()
    bad["kind"][len(bad) // 2] = 7
    assert RP.replay(st.copy(), tt, tc, bad, R=R, cap=cap, seed=1, step=0, emin=5000, emax=10000)["malformed"] >= 1


def blank_state(G):
    from helpers import blank_groups
    return blank_groups(G, R)
