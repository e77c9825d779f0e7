"""The trackers' launch-order ladder and tail class (csrc/klt_sched.h) on the CPU: klt_sched_step, klt_tail_class_step and
klt_tail_next_call are pure functions of (state, values), walked here without a device through host/build/klt_sched_cli — against
an independent restatement of the code they were lifted from (tests/klt_sched_ref.py) over random call sequences, and on the named
sequences that used to exist only as comments."""
import os
import random
import subprocess

from tests import klt_sched_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "klt_sched_cli")

BASIC, AFFINE, LSSD = 0, 1, 2
INVERSE, DIRECT, FAST, NEON = 0, 1, 2, 4
NOT_SET = -1
MIN_FEATURES, MIN_LONG_TAIL, MAX_FEATURES = 4096, 1024, 1 << 18  # kSchedMinFeatures, kSchedMinLongTail, kSchedMaxFeatures
TAIL_HOLD = 8                                                    # kTailHold


def cli(lines):
    """One output dict per command that prints (everything but new / set / fail)."""
    assert os.path.exists(EXE), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = {}
        for kv in line.split():
            k, v = kv.split("=")
            d[k] = int(v) if v.lstrip("-").isdigit() else v
        out.append(d)
    assert len(out) == sum(1 for l in lines if l.split()[0] not in ("new", "set", "fail"))
    return out


def call(n, n_track=None, model=LSSD, waves=1, long_tail=0, capturing=0, ref_untouched=1, sched=NOT_SET, sched_min=NOT_SET, have=(1, 1, 1)):
    return dict(n=n, n_track=n if n_track is None else n_track, model=model, waves=waves, long_tail=long_tail, capturing=capturing, ref_untouched=ref_untouched,
                sched=sched, sched_min=sched_min, have_grid=have[0], have_claim=have[1], have_pred=have[2])


def call_line(c):
    return "call " + " ".join(str(c[k]) for k in ("n", "n_track", "model", "waves", "long_tail", "capturing", "ref_untouched", "sched", "sched_min", "have_grid",
                                                   "have_claim", "have_pred"))


def steps(calls, first=("new",)):
    return cli(list(first) + [c if isinstance(c, str) else call_line(c) for c in calls])


# ---------------------------------------------------------------------------------------------------------------------------------
# against the independent restatement
# ---------------------------------------------------------------------------------------------------------------------------------
N_VALUES = (1, 300, 1023, 1024, 1025, 1536, 1537, 4095, 4096, 4097, 8192, 262144, 262145)


def random_sequence(rng, length=50):
    """(commands for the CLI, the restatement's answers): calls with runs of equal n, failed launches (each followed by the reset)."""
    model_state = ref.Sched()
    lines, expected = ["new"], []
    if rng.random() < 0.15:  # now and then near the wrap of the claim tag
        start = 0x7FFFFF - rng.randrange(0, 40) + rng.choice((0, 1 << 23, 0xFF800000))
        lines.append(f"set sched_call {start}")
        model_state.sched_call = start
    n = rng.choice(N_VALUES)
    while len(expected) < length:
        if rng.random() < 0.3:
            n = rng.choice(N_VALUES)
        have = (1, 1, 1) if rng.random() < 0.9 else tuple(rng.randrange(2) for _ in range(3))
        c = call(n, n_track=rng.choice((n, n, n, min(n, 500), max(n - 1, 0))), model=rng.randrange(3), waves=rng.randint(1, 4), long_tail=rng.randrange(2),
                 capturing=int(rng.random() < 0.15), ref_untouched=int(rng.random() < 0.8), sched=rng.choice((NOT_SET, NOT_SET, 0, 1)),
                 sched_min=rng.choice((NOT_SET, NOT_SET, 0, 1024, 100000)), have=have)
        lines.append(call_line(c))
        expected.append(model_state.call(c["n"], c["n_track"], c["model"], c["waves"], c["long_tail"], c["capturing"], c["ref_untouched"], c["sched"], c["sched_min"],
                                         c["have_grid"], c["have_claim"], c["have_pred"]))
        if rng.random() < 0.05:
            lines.append("fail")
            model_state.reset()
    return lines, expected


def test_random_call_sequences_equal_the_restatement_field_by_field():
    rng = random.Random(20261017)
    lines, expected, starts = [], [], []
    for s in range(240):
        l, e = random_sequence(rng)
        starts.append(len(expected))
        lines += l
        expected += e
    got = cli(lines)
    seen_orders = set()
    for i, (g, e) in enumerate(zip(got, expected)):
        seq = max(k for k, at in enumerate(starts) if at <= i)
        assert g == e, f"sequence {seq}, call {i - starts[seq]}: library {g} != restatement {e}"
        seen_orders.add((g["order"], g["trades"], g["wipe"], g["grow_to"] != 0))
    # the sequences reach every kind of step
    assert {o for o, _, _, _ in seen_orders} == {"none", "index", "position"}
    assert any(t for _, t, _, _ in seen_orders) and any(w for _, _, w, _ in seen_orders) and any(gr for _, _, _, gr in seen_orders)


def test_random_tail_sequences_equal_the_restatement():
    rng = random.Random(7)
    lines, expected, sequence = [], [], []
    for s in range(200):
        model_state = ref.Tail()
        lines.append("new")
        if rng.random() < 0.3:
            start = 0xFFFFFF - rng.randrange(0, 300)
            lines.append(f"set tail_call {start}")
            model_state.tail_call = start
        for _ in range(60):
            model, method = rng.randrange(3), rng.choice((INVERSE, DIRECT, FAST, NEON))
            age = rng.choice((0, 1, 255, 256, 257, 1000, 0xFFFFFF))
            seen = rng.choice((0, (((model_state.tail_call - age) & 0xFFFFFF) << 8) | rng.choice((0, 1, 12, 23, 24, 25, 255))))
            lines.append(f"tail {model} {method} {seen}")
            expected.append(dict(long_tail=model_state.class_of(model, method, seen)))
            lines.append(f"launch {model} {method}")
            number, wipe = model_state.next_call(model, method)
            expected.append(dict(tail_call=number, wipe=wipe))
            sequence += [s, s]
    for i, (g, e) in enumerate(zip(cli(lines), expected)):
        assert g == e, f"sequence {sequence[i]}, step {i - sequence.index(sequence[i])}: library {g} != restatement {e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# named sequences
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ladder_at_constant_n():
    s = steps([call(5000, model=BASIC)] * 5)
    assert [x["iters_buf"] for x in s] == [0, 1, 0, 1, 0]
    assert [x["sort_from"] for x in s] == [-1, 0, 1, 0, 1]  # the sort of call k orders iters[sort_from] into order[sort_from]
    assert [x["order"] for x in s] == ["none", "none", "index", "index", "index"]
    assert [x["order_buf"] for x in s[2:]] == [0, 1, 0]
    for k in range(2, 5):
        assert s[k]["order_buf"] == s[k - 1]["sort_from"]  # installed at call k: written by the sort of call k - 1 ...
        assert s[k - 1]["sort_from"] == s[k - 2]["iters_buf"]  # ... from the counts of call k - 2
        assert s[k]["order_buf"] != s[k]["sort_from"]  # and nobody writes it during call k
    assert [x["grow_to"] for x in s] == [8192, 0, 0, 0, 0] and all(x["sort_reads_ref_uv"] == 1 for x in s[1:])
    assert [x["sched_call"] for x in s] == [5, 6, 7, 8, 9] and all(x["recording"] and x["active"] for x in s)


def test_a_changed_n_restarts_the_ladder_and_gets_the_position_order():
    base = [call(5000)] * 3
    s = steps(base + [call(4500), call(4500), call(4500)])
    assert [x["order"] for x in s] == ["none", "position", "index", "position", "position", "index"]
    assert [x["iters_buf"] for x in s[3:]] == [0, 1, 0] and s[3]["sort_from"] == -1 and s[3]["order_buf"] == 0 and s[4]["order_buf"] == 1
    # ... exactly when: recording, the last call recorded under the preceding number, not Basic, no trades, a prediction buffer
    assert steps(base + [call(4500, capturing=1)])[3]["order"] == "none"
    assert steps(base + [call(4500, model=BASIC)])[3]["order"] == "none"
    assert steps(base + [call(4500, waves=2)])[3]["order"] == "none" and steps(base + [call(4500, waves=2)])[3]["trades"] == 1
    assert steps(base + [call(4500, waves=2, ref_untouched=0)])[3]["order"] == "position"  # no trades: the order instead
    assert steps(base + [call(4500, have=(1, 1, 0))])[3]["order"] == "none"
    assert steps(base + [call(4500, have=(0, 1, 1))])[3] ["order"] == "none"
    assert steps([call(4500)])[0]["order"] == "none"  # nothing recorded yet


def test_a_capturing_call_does_not_record():
    s = steps([call(5000, waves=2), call(5000, waves=2), call(5000, waves=2, capturing=1)])
    cap = s[2]
    assert (cap["recording"], cap["trades"], cap["sched_call"]) == (0, 0, 0)
    assert cap["state_call"] == s[1]["state_call"] == 6 and cap["state_recorded"] == 6  # neither counter moved
    assert cap["order"] == "index"  # the ladder itself goes on: the order was made by a launch outside the capture
    cap_first = steps([call(5000), call(4500, capturing=1)])[1]
    assert (cap_first["order"], cap_first["recording"]) == ("none", 0)


def test_first_call_after_a_capture_documents_current_behaviour():
    """DOCUMENTS CURRENT BEHAVIOUR: a capturing call advances neither the call number nor `recorded`, so for the
    first call after it `last recorded + 1 == this call` still holds and it DOES get the position order — from the table of the last
    call outside the capture, however many captured calls (and their replays) lie in between.  The order is a heuristic and the table
    is intact, so no result depends on it; whether a table that old should still count is a question for the change that makes the
    position order the only one."""
    s = steps([call(5000), call(5000), call(5000, capturing=1), call(4500), call(4500)])
    assert (s[3]["recording"], s[3]["sched_call"], s[3]["order"]) == (1, 7, "position")  # 6 + 1 == 7
    s = steps([call(5000), call(5000, capturing=1), call(4500, capturing=1), call(4500)])
    assert s[3]["order"] == "position" and s[3]["sched_call"] == 6
    # what does break the chain is a call number that moved without a recording
    s = steps([call(5000), "set sched_call 9", call(4500)])
    assert s[1]["sched_call"] == 10 and s[1]["order"] == "none"


def test_results_written_over_the_reference_positions():
    s = steps([call(5000, waves=2, ref_untouched=0)] * 3)
    assert all(x["trades"] == 0 for x in s)
    assert [x["sort_reads_ref_uv"] for x in s] == [0, 0, 0] and [x["sort_from"] for x in s] == [-1, 0, 1]
    assert s[2]["order"] == "index" and s[2]["order_buf"] == 0
    assert [x["trades"] for x in steps([call(5000, waves=2)] * 2)] == [1, 1]
    assert [x["trades"] for x in steps([call(5000, waves=1)] * 2)] == [0, 0]  # multi-wave features only
    assert [steps([call(n, waves=2, long_tail=1)])[0]["trades"] for n in (1536, 1537)] == [0, 1]  # late slot + head first + head slots


def test_threshold_selection():
    def active(**kw):
        return steps([call(**kw)])[0]["active"]
    assert [active(n=MIN_FEATURES - 1), active(n=MIN_FEATURES)] == [0, 1]
    assert [active(n=9000, n_track=MIN_FEATURES - 1), active(n=9000, n_track=MIN_FEATURES)] == [0, 1]  # the tracked features count
    assert [active(n=MIN_LONG_TAIL - 1, long_tail=1), active(n=MIN_LONG_TAIL, long_tail=1), active(n=MIN_LONG_TAIL, long_tail=0)] == [0, 1, 0]
    assert [active(n=MAX_FEATURES), active(n=MAX_FEATURES + 1)] == [1, 0]
    assert [active(n=9000, sched=0), active(n=9000, sched=1)] == [0, 1]
    assert [active(n=300, sched_min=0), active(n=1023, sched_min=1024), active(n=9000, sched_min=100000), active(n=100000, sched_min=100000)] == [1, 0, 0, 1]
    off = steps([call(9000), call(9000, sched=0), call(9000), call(9000)])
    assert off[1] == dict(off[1], active=0, order="none", sort_from=-1, recording=0, sched_call=0, trades=0, grow_to=0, wipe=0)
    assert off[1]["state_calls"] == 1 and [x["order"] for x in off] == ["none", "none", "position", "index"]  # an inactive call leaves the state alone


def test_claim_tag_wrap():
    start = 0x7FFFFF - 2
    s = steps([call(5000, waves=2)] * 6, first=("new", f"set sched_call {start}"))
    assert [x["sched_call"] for x in s] == [start + 1, start + 2, start + 7, start + 8, start + 9, start + 10]  # ... jumps by 4 over the tags 0 .. 3
    assert [x["wipe"] for x in s] == [0, 0, 1, 0, 0, 0]
    assert all((x["sched_call"] & 0x7FFFFF) >= 4 for x in s)
    # the wiping call forgets what was recorded (its tables are gone): no position order for it
    s = steps([call(5000), call(5000), call(4500), call(4500)], first=("new", f"set sched_call {start}"))
    assert [x["wipe"] for x in s] == [0, 0, 1, 0] and [x["order"] for x in s] == ["none", "position", "none", "position"]


def test_capacity_growth():
    s = steps([call(4097), call(4097), call(4097), call(8192), call(8192), call(8193), call(5000), call(5000), call(5000)])
    assert [x["grow_to"] for x in s] == [8192, 0, 0, 0, 0, 12288, 0, 0, 0]
    assert [x["state_capacity"] for x in s] == [8192] * 5 + [12288] * 4
    assert [x["state_calls"] for x in s] == [1, 2, 3, 1, 2, 1, 1, 2, 3]
    assert s[5]["sort_from"] == -1 and s[5]["iters_buf"] == 0  # a growth restarts the ladder
    assert steps([call(4096)])[0]["grow_to"] == 4096
    # a growth brings every buffer with it
    assert steps([call(5000, have=(0, 0, 0))])[0]["recording"] == 1
    # the launch of the second call fails: the third must not install an order nobody wrote
    s = steps([call(5000), call(5000), "fail", call(5000), call(5000), call(5000)])
    assert [x["order"] for x in s] == ["none", "position", "position", "position", "index"] and s[2]["sort_from"] == -1


def tail_word(call_number, iters):
    return (call_number << 8) | iters


def test_tail_class_freshness_and_hold():
    def class_after(age, iters):
        lines = ["new"] + ["launch 2 2"] * 300 + [f"tail 2 2 {tail_word(300 - age, iters)}"]
        return cli(lines)[-1]["long_tail"]
    assert [class_after(0, 24), class_after(256, 24), class_after(257, 24)] == [1, 1, 0]
    assert [class_after(0, 23), class_after(0, 255)] == [0, 1]
    assert cli(["new", "launch 2 2", "tail 2 2 0"])[-1]["long_tail"] == 0  # nothing reported yet
    # one long report holds for kTailHold launches of THAT variant: launches of another one do not use it up
    lines = ["new", "launch 2 2", f"tail 2 2 {tail_word(1, 30)}"]
    for _ in range(TAIL_HOLD):
        lines += ["launch 1 0", "launch 2 2", "tail 2 2 0"]
    got = [d["long_tail"] for d in cli(lines) if "long_tail" in d]
    assert got == [1] * TAIL_HOLD + [0]
    assert cli(["new", "launch 2 2", f"tail 2 2 {tail_word(1, 30)}", "tail 1 0 0", "tail 2 0 0"])[-2:] == [dict(long_tail=0), dict(long_tail=0)]
    # sse / neon share the fast variant's state
    assert cli(["new", "launch 2 4", f"tail 2 2 {tail_word(1, 30)}", "tail 2 3 0"])[-1]["long_tail"] == 1


def test_tail_call_wrap():
    got = cli(["new", "set tail_call 16777213", "launch 0 0", "launch 0 0", "launch 0 0", "launch 0 0"])
    assert got == [dict(tail_call=0xFFFFFE, wipe=0), dict(tail_call=0xFFFFFF, wipe=0), dict(tail_call=1, wipe=1), dict(tail_call=2, wipe=0)]
    # a report from just before the wrap is still one launch old, not 16 M
    got = cli(["new", "set tail_call 16777214", "launch 0 0", f"tail 0 0 {tail_word(0xFFFFFF, 40)}"])
    assert got[-1]["long_tail"] == 1


def test_word_helpers_round_trip_at_the_field_limits():
    for kind, call_bits, low_max in (("grid", 24, 255), ("claim", 23, 0x1FF), ("flag", 31, 1), ("tail", 24, 255)):
        top = (1 << call_bits) - 1
        cases = [(c, l) for c in (0, 1, 4, top - 1, top) for l in (0, 1, low_max - 1, low_max)]
        got = cli([f"word {kind} {c} {l}" for c, l in cases])
        for (c, l), g in zip(cases, got):
            assert (g["call"], g["low"]) == (c, l), (kind, c, l, g)
            assert g["word"] == (c << (32 - call_bits)) | l
    # iteration counts saturate at 255; a call number beyond its field is cut to it (the tail word's is kept in 24 bits by its counter)
    assert cli(["word grid 5 300", "word grid 16777221 7", "word claim 8388613 511"]) == [dict(word=(5 << 8) | 255, call=5, low=255), dict(word=(5 << 8) | 7, call=5, low=7),
                                                                                         dict(word=(5 << 9) | 511, call=5, low=511)]
