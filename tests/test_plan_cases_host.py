"""CPU check of tests/plan_cases.py: every case of the table plans and packs on the host, and the table holds a case for every
launch sequence an alternative plan takes over the sizes and class counts the default plan is tested at (the host-only dry run,
yfv2_debug_plan_image_ex: step -1 = the number of steps, then each step's name, HxW figures removed).  A change of a static bound
that gives some shape a new sequence of launches fails here until tests/plan_cases.py has a case that runs it on the device."""
import pytest

import plan_cases as P


def _table_sequences(plan):
    return {P.launch_sequence(c.plan, c.classes, c.H, c.W) for c in P.CASES if c.kind == "forward" and c.plan == plan}


def test_every_case_of_the_table_dry_runs():
    ids = [P.case_id(c) for c in P.CASES]
    assert len(set(ids)) == len(ids), "two cases share an id"
    seqs = P.launch_sequences((c.plan, c.classes, c.H, c.W) for c in P.CASES)      # asserts rc 0 of every dry run
    for c, names in zip(P.CASES, seqs):
        assert len(names) >= 12, "%s: %d launches" % (P.case_id(c), len(names))
        assert c.kind in ("forward", "batch", "post") and c.B >= 3 and (c.kind != "batch" or c.B % 3 == 0)
        if c.kind == "post":    # the default handle must take the fused launch: that is what the two-launch form is compared with
            assert c.classes <= 96 and 3 * ((c.H // 16) * (c.W // 16) + (c.H // 32) * (c.W // 32)) <= 2048, P.case_id(c)


@pytest.mark.parametrize("plan", P.COVERED_PLANS, ids=P.plan_name)
def test_table_covers_every_launch_sequence_of_the_plan(plan):
    seqs = P.sequences_over_lists(plan)
    have = _table_sequences(plan)
    missing = [cfgs for s, cfgs in seqs.items() if s not in have]
    assert not missing, "%s: %d of %d launch sequences have no case in tests/plan_cases.py; they occur at (H, W, classes) %s" % (
        P.plan_name(plan), len(missing), len(seqs), [m[:4] for m in missing])


def test_table_covers_every_sequence_towers_unpaired_changes():
    default = {c: s for s, cfgs in P.sequences_over_lists({}).items() for c in cfgs}
    seqs = P.sequences_over_lists(P.UNPAIRED)
    have = _table_sequences(P.UNPAIRED)
    changed = {s: [c for c in cfgs if default[c] != s] for s, cfgs in seqs.items()}
    changed = {s: cfgs for s, cfgs in changed.items() if cfgs}
    assert changed, "towers_unpaired changes no launch sequence: the switch is not read"
    missing = [cfgs for s, cfgs in changed.items() if s not in have]
    assert not missing, "towers_unpaired: %d of %d changed launch sequences have no case; they occur at (H, W, classes) %s" % (
        len(missing), len(changed), [m[:4] for m in missing])
    for c in P.CASES:    # and every towers_unpaired case is one the switch changes (it is compared bit for bit with the default plan)
        if c.plan == P.UNPAIRED:
            assert P.launch_sequence(P.UNPAIRED, c.classes, c.H, c.W) != P.launch_sequence({}, c.classes, c.H, c.W), P.case_id(c)
