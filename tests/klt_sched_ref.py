"""A plain-Python model of the trackers' two host-side state machines: which launch order a call gets (the
ladder) and which tail class a variant is in.  Restated from klt_sched_prepare / klt_tail_class / klt_tail_number as they stood in
ftk_klt.cpp before they became step functions, statement by statement, with that file's literals: it shares no constant with
csrc/klt_sched.h.  tests/test_klt_sched_cpu.py compares the library's step functions with it; tests/test_klt_gpu.py asks it from
which call on a launch order is installed."""

BASIC = 0
NOT_SET = -1
M32 = 0xFFFFFFFF


class Sched:
    """The context's counters and one call of klt_sched_prepare."""

    def __init__(self):
        self.sched_recorded = 0
        self.sched_call = 0
        self.sched_capacity = 0
        self.sched_n = 0
        self.sched_calls = 0

    def reset(self):
        """'the history starts over' (a large-patch call, a failed launch)"""
        self.sched_calls = 0
        self.sched_n = 0

    def call(self, n, n_track, model, waves, long_tail, capturing, ref_untouched, sched=NOT_SET, sched_min=NOT_SET, have_grid=1, have_claim=1, have_pred=1):
        out = dict(active=0, grow_to=0, wipe=0, iters_buf=0, sort_from=-1, sort_reads_ref_uv=0, order="none", order_buf=0, recording=0, sched_call=0, trades=0)
        sched_allowed = not (sched != NOT_SET and sched == 0)
        threshold = sched_min if sched_min != NOT_SET else (1024 if long_tail else 4096)
        if sched_allowed and n_track >= threshold and n <= (1 << 18):
            out["active"] = 1
            if n > self.sched_capacity:
                self.sched_capacity = 0
                self.sched_n = 0
                cap = (n + 4095) // 4096 * 4096
                have_grid = have_claim = have_pred = 1  # every buffer is reserved here
                out["grow_to"] = cap
                self.sched_capacity = cap
            if self.sched_n != n:
                self.sched_n = n
                self.sched_calls = 0
            k = self.sched_calls
            self.sched_calls += 1
            recording = (not capturing) and have_grid and have_claim
            last_recorded = 0
            if recording:
                if self.sched_call < 4:
                    self.sched_call = 4
                self.sched_call = (self.sched_call + 1) & M32
                if (self.sched_call & 0x7FFFFF) < 4:
                    out["wipe"] = 1
                    self.sched_call = (self.sched_call + 4) & M32
                    self.sched_recorded = 0
                out["recording"] = 1
                out["sched_call"] = self.sched_call
                last_recorded = self.sched_recorded
                self.sched_recorded = self.sched_call
            claim_installed = bool(recording and waves >= 2 and ref_untouched and n > 1024 + 512)
            out["trades"] = int(claim_installed)
            out["iters_buf"] = k & 1
            if k >= 1:
                out["sort_from"] = (k - 1) & 1
                out["sort_reads_ref_uv"] = int(bool(ref_untouched))
            if k >= 2:
                out["order"], out["order_buf"] = "index", k & 1
            elif recording and last_recorded != 0 and ((last_recorded + 1) & M32) == self.sched_call and have_pred and model != BASIC and not claim_installed:
                out["order"], out["order_buf"] = "position", k & 1
        out.update(state_recorded=self.sched_recorded, state_call=self.sched_call, state_capacity=self.sched_capacity, state_n=self.sched_n,
                   state_calls=self.sched_calls)
        return out


class Tail:
    """tail_call and the per-variant launch counts: klt_tail_class (class_of) and klt_tail_number (next_call)."""

    def __init__(self):
        self.tail_call = 0
        self.launches = {}
        self.long_until = {}

    @staticmethod
    def _variant(model, method):
        return (model, 0 if method == 0 else (1 if method == 1 else 2))

    def class_of(self, model, method, seen):
        v = self._variant(model, method)
        launches = self.launches.get(v, 0)
        age = (self.tail_call - (seen >> 8)) & 0xFFFFFF
        if seen != 0 and age <= 256 and (seen & 0xFF) >= 24:
            self.long_until[v] = (launches + 8) & M32
        return 1 if launches < self.long_until.get(v, 0) else 0

    def next_call(self, model, method):
        self.tail_call = (self.tail_call + 1) & 0xFFFFFF
        wipe = 0
        if self.tail_call == 0:
            self.tail_call = 1
            wipe = 1
        v = self._variant(model, method)
        self.launches[v] = (self.launches.get(v, 0) + 1) & M32
        return self.tail_call, wipe
