"""CPU tier of the crowd tests: the conditions on the inputs of tests/test_crowd_gpu.py (tests/crowd_cases.py), so that the GPU
tier cannot be about less than it claims, and the Python schedule against a step-by-step walk of its own definition."""
import crowd_cases as cc


def test_the_calls_and_the_cuts():
    segs = cc.segments()
    assert sum(n for _, n in segs) == cc.END - cc.START == 48 and segs[0][0] == cc.START
    assert all(a + n == b for (a, n), (b, _) in zip(segs, segs[1:]))  # (contiguous)
    print(cc.census(segs))
    assert len(segs) == 22
    lengths = [n for _, n in segs]
    assert 1 in lengths and 2 in lengths and max(lengths) >= 3
    # a walk step by step: a segment ends where a call ends or a joined consumer is due, and nowhere else
    ends, c = set(cc.call_ends()), cc.START
    for c0, n in segs:
        assert c0 == c
        for s in range(c0 + 1, c0 + n):
            assert s not in ends and all(s % e for e in cc.JOINED.values()), s
        c = c0 + n
        assert c in ends or any(c % e == 0 for e in cc.JOINED.values()), c
    # the compact longwave record is entered from every phase of the shortwave cycle
    for phase in range(3):
        assert any(c0 % 3 == phase and n >= 2 for c0, n in segs), phase


def test_the_periods_are_pairwise_non_commensurate_where_the_feature_allows():
    d, v, q = cc.DRIVER_EVERY, cc.VERIF_EVERY, cc.QTAPE_EVERY
    assert len({d, v, q}) == 3 and all(a % b for a in (d, v, q) for b in (d, v, q) if a != b)
    assert cc.EVERY["tape"] == 1  # (the arbiters' input: every step)
    assert cc.START % v and cc.START % q and cc.END % v and cc.END % q  # (the calls begin and end between their events)
    assert cc.NUDGE_STAMPS[0] < cc.START and cc.NUDGE_STAMPS[1] > cc.END + len(cc.OFF_ORDER) * cc.EXTRA


def test_cuts_due_for_two_and_for_three_joined_consumers():
    cuts = [c0 + n for c0, n in cc.segments()]
    n_due = {c: sum(1 for e in cc.JOINED.values() if c % e == 0) for c in cuts}
    assert 2 in n_due.values() and 3 in n_due.values() and 1 in n_due.values() and 0 in n_due.values()
    assert [c for c, k in n_due.items() if k == 3] == [36, 72]
    assert cc.events_at(36, "B") == ["qtape", "verif0", "analysis", "verif1"]
    assert cc.events_at(72, "B") == ["qtape", "verif0", "analysis", "verif1"]
    assert cc.events_at(60, "B") == ["verif0", "skipped"] and cc.events_at(54, "B") == ["qtape", "skipped"]
    assert cc.events_at(72, "A") == ["qtape", "verif0", "rescale"]
    assert cc.events_at(42, "B") == ["analysis"] and cc.events_at(45, "A") == ["qtape"] and cc.events_at(35, "A") == []


def test_cuts_inside_open_windows():
    cuts = [c0 + n for c0, n in cc.segments()][:-1]
    acc, _ = cc.window_rows(cc.EVERY["acctape"], cc.START, cc.END)
    win, _ = cc.window_rows(cc.EVERY["wintape"], cc.START, cc.END, cc.WIN_SAMPLE_EVERY)

    def strictly_inside(cut, rows):
        return any(n - steps < cut < n for n, _, steps in rows)

    assert any(strictly_inside(c, acc) for c in cuts) and any(strictly_inside(c, win) for c in cuts)
    # ... and one cut inside both at once, between two shortwave steps
    both = [c for c in cuts if strictly_inside(c, acc) and strictly_inside(c, win) and c % 3]
    assert both, both
    # the first windows are short, the later ones whole; the accumulation tape's last window is still open at the end
    assert acc[0] == (32, 2, 2) and all(r[2] == cc.EVERY["acctape"] for r in acc[1:])
    assert win[0] == (36, 3, 6) and all(r[1:] == (3, 6) for r in win)
    assert cc.window_rows(cc.EVERY["acctape"], cc.START, cc.END)[1] == (76, 2)
    assert cc.window_rows(cc.EVERY["wintape"], cc.START, cc.END, cc.WIN_SAMPLE_EVERY)[1] == (78, 0)


def test_every_small_ring_wraps_inside_a_segment_and_across_a_cut():
    inside = across = 0
    for driver in ("A", "B"):
        for name in cc.SMALL:
            if name == ("assim" if driver == "A" else "breed"):
                continue
            steps = cc.ring_steps(name, driver)
            assert len(steps) > cc.CAPACITY[name], (name, steps)
            i, a = cc.wraps(name, driver)
            assert i + a >= 1, name
            inside, across = inside + i, across + a
    assert inside >= 1 and across >= 1
    assert cc.wraps("projtape") == (2, 2)  # 50 -> 52 and 70 -> 72 inside a segment; 40 | 42 and 60 | 62 across a cut
    assert len(cc.ring_steps("tape")) == cc.CAPACITY["tape"]  # (the arbiters' input holds every step)
    # the case without a joined consumer: every small ring of a recorder wraps inside its only segment
    solo = cc.segments(cc.START, (cc.SOLO_CALL,), ())
    for name in ("spectra", "enstape", "acctape", "wintape", "projtape"):
        i, a = cc.wraps(name, "A", cc.START, cc.START + cc.SOLO_CALL, solo)
        assert i >= 1 and a == 0, name


def test_analyses_applied_and_skipped_and_the_second_phase():
    events = cc.due(cc.DRIVER_EVERY, cc.START, cc.END)
    applied = [s for s in events if s in cc.ROWS]
    assert applied == cc.ring_steps("assim", "B") == list(cc.ROWS) and len(applied) < len(events)
    scored = cc.due(cc.VERIF_EVERY, cc.START, cc.END)
    second = [s for s in scored if "verif1" in cc.events_at(s, "B")]
    cuts_of_both = [s for s in scored if s % cc.DRIVER_EVERY == 0]
    assert second == [36, 72] and set(second) < set(cuts_of_both)
    # ... and the quantile tape's ring still holds a sample taken in front of an analysis that was applied
    assert any("analysis" in cc.events_at(s, "B") for s in cc.held(cc.ring_steps("qtape", "B"), "qtape"))
    assert any("verif1" in cc.events_at(s, "B") for s in cc.held(scored, "verif"))       # the ring still holds a filled phase 1
    assert any(s % cc.DRIVER_EVERY == 0 and "verif1" not in cc.events_at(s, "B") for s in cc.held(scored, "verif"))
    assert not any("verif1" in cc.events_at(s, "A") for s in scored)


def test_the_call_without_a_joined_consumer_is_one_long_segment():
    segs = cc.segments(cc.START, (cc.SOLO_CALL,), ())
    assert segs == [(cc.START, cc.SOLO_CALL)] and cc.SOLO_CALL >= cc.OFFSET_FROM
    assert all(n < cc.OFFSET_FROM for _, n in cc.segments())  # (and no segment of the crowd's calls takes that path)


def test_plans_masks_and_entries():
    assert {plan for plan, _ in cc.CASES} == set(cc.PLANS)
    assert set(cc.CASES) == {("serial_5", "A"), ("groups_rounds_12", "A"), ("groups_rounds_12", "B"), ("fp32_storage_6", "B")}

    def contiguous(mask):
        on = cc.masked(mask)
        return on == list(range(on[0], on[-1] + 1))

    for key, plan in cc.PLANS.items():
        M = plan["members"]
        (vmask, truth), qmask = plan["verif"], plan["qtape"]
        masks = [vmask, qmask] + ([plan["assim"]] if plan["assim"] else [])
        assert all(len(m) == M and not contiguous(m) and 2 <= sum(m) for m in masks), key
        assert len({tuple(m) for m in masks}) == len(masks), key
        assert vmask[truth] == 0
        if plan["control"]:
            ctl = plan["control"]
            controls = sorted({c for c in ctl if c >= 0})
            assert len(ctl) == M and len(controls) == 2 and all(ctl[c] == -1 for c in controls)
            sizes = [sum(1 for c in ctl if c == k) for k in controls]
            assert max(sizes) == 2  # (a family of two: Gram-Schmidt has something to do; five members leave one for the other)
            assert sizes == [2, 2] or M < 6
    plan = cc.PLANS["groups_rounds_12"]
    block, groups = dict(plan["options"])["block_members"], dict(plan["options"])["member_groups"]
    per_round = block * groups
    truth = plan["verif"][1]
    assert truth // per_round == (plan["members"] - 1) // per_round and (truth % per_round) // block == 1  # last round, second group
    bred = [i for i, c in enumerate(plan["control"]) if c >= 0]
    assert any(i // per_round != plan["control"][i] // per_round for i in bred)  # a control in another round
    assert plan["members"] > 8 and cc.PLANS["serial_5"]["members"] % 2 == 1
    assert cc.PLANS["fp32_storage_6"]["fp32"] and not plan["fp32"]
    # the entries, between them
    lists = (cc.PROJTAPE, cc.VERIF, cc.QTAPE)
    for entries in lists:
        planes = {e[:2] for e in entries}
        assert {("t_grid", 0), ("t_grid", 7), ("ps_grid", 0), ("precnv", 0), ("precls", 0), ("mslp", 0), ("z_plev", 0), ("tcwv", 0)} <= planes
        assert {e[0] for e in entries} <= set(cc.TAPED)  # (the arbiters read every plane from the crowd's own tape)
    assert cc.VERIF[cc.VERIF_PRECNV][0] == cc.QTAPE[cc.QTAPE_PRECNV][0] == cc.QTAPE[cc.QTAPE_PRECNV_Q][0] == "precnv"
    assert not {"precnv", "precls"} & {e[0] for e in cc.ASSIM}
    assert set(cc.DERIVE_TAPED + cc.PLEV_TAPED) < set(cc.TAPED)
    assert {n for n, *_ in cc.ACCTAPE} >= {"precnv", "precls"} and "precnv" in cc.STATS and "precnv" in {e[0] for e in cc.WINTAPE}
    assert set(cc.OFF_ORDER) | {"derive", "plev"} == set(cc.CONSUMERS) and len(cc.CONSUMERS) == 11
