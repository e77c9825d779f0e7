"""A numpy restatement of the landmark table's query and update (include/ftk.h): TEST INFRASTRUCTURE, never imported by the
package.  Written from the contract, for reading: sequential loops over rows and slots, integer logic and copies, so equality with the
device is exact.  ``mutant`` names one deliberate mistake (tests/test_match_table_ref_cpu.py shows that each is caught)."""
import numpy as np

NOT_TRACKED, TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR = range(5)
MUTANTS = ("admit_descending", "retire_at_max_lost", "admit_rejected", "highest_row_wins", "keep_old_descriptor")
FIELDS = ("ids", "points", "prev_points", "descriptors", "status", "age", "lost", "n_live", "next_id")


def clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


class Table:
    """The nine tensors of the landmark table as numpy arrays."""

    def __init__(self, n, dim, next_id=0):
        self.n, self.dim = int(n), int(dim)
        self.next_id = np.array([next_id], np.int64)
        self.empty()

    def empty(self):
        n = self.n
        self.ids = np.full(n, -1, np.int64)
        self.points = np.zeros((n, 2), np.float32)
        self.prev_points = np.zeros((n, 2), np.float32)
        self.descriptors = np.zeros((n, self.dim), np.float32)
        self.status = np.full(n, OUTSIDE, np.uint8)
        self.age = np.zeros(n, np.int32)
        self.lost = np.zeros(n, np.int32)
        self.n_live = np.zeros(1, np.int32)

    def tensors(self):
        return {k: getattr(self, k) for k in FIELDS}

    def copy(self):
        other = Table(self.n, self.dim)
        for k in FIELDS:
            setattr(other, k, getattr(self, k).copy())
        return other

    def query(self):
        """(q_uv [n, 2], q_desc [n, D], q_slot [n], q_count [1]): the live slots in ascending slot order, +0 and -1 behind them."""
        q_uv = np.zeros((self.n, 2), np.float32)
        q_desc = np.zeros((self.n, self.dim), np.float32)
        q_slot = np.full(self.n, -1, np.int32)
        nq = 0
        for s in range(self.n):
            if self.ids[s] >= 0:
                q_uv[nq], q_desc[nq], q_slot[nq] = self.points[s], self.descriptors[s], s
                nq += 1
        return q_uv, q_desc, q_slot, np.array([nq], np.int32)

    def update(self, q_slot, q_count, match_index, match_status, cur_uv, cur_desc, cur_count, max_lost, mutant=None):
        """One frame's results into the table; returns cur_slot [K]."""
        cur_uv = np.asarray(cur_uv, np.float32).reshape(-1, 2)
        K = cur_uv.shape[0]
        nq = clamp(q_count, 0, self.n)
        nk = K if cur_count is None else clamp(cur_count, 0, K)
        # 1. claiming
        names = [int(match_index[r]) if 0 <= int(match_index[r]) < nk else None for r in range(nq)]
        claimed = {j for j in names if j is not None}
        winner = {}
        for r in (reversed(range(nq)) if mutant == "highest_row_wins" else range(nq)):
            j = names[r]
            if j is not None and int(match_status[r]) == TRACKED and j not in winner:
                winner[j] = r
        if mutant == "admit_rejected":
            claimed = set(winner)
        cur_slot = np.full(K, -1, np.int32)
        # 2. the live slots
        was_empty = self.ids < 0
        for r in range(nq):
            s = int(q_slot[r])
            if not 0 <= s < self.n or was_empty[s]:
                continue
            j = names[r]
            if j is not None and winner.get(j) == r:
                self.prev_points[s] = self.points[s]
                self.points[s] = cur_uv[j]
                if mutant != "keep_old_descriptor":
                    self.descriptors[s] = cur_desc[j]
                self.age[s] += 1
                self.lost[s] = 0
                self.status[s] = TRACKED
                cur_slot[j] = s
            else:
                self.lost[s] += 1
                self.status[s] = LARGE_RESIDUAL
                if (self.lost[s] >= max_lost) if mutant == "retire_at_max_lost" else (self.lost[s] > max_lost):
                    self.ids[s] = -1
        # 3. admission
        unclaimed = [j for j in range(nk) if j not in claimed]
        if mutant == "admit_descending":
            unclaimed.reverse()
        empty = [s for s in range(self.n) if self.ids[s] < 0]
        admitted = min(len(unclaimed), len(empty))
        for rank in range(admitted):
            j, s = unclaimed[rank], empty[rank]
            self.ids[s] = self.next_id[0] + rank
            self.points[s] = cur_uv[j]
            self.prev_points[s] = cur_uv[j]
            self.descriptors[s] = cur_desc[j]
            self.age[s] = 0
            self.lost[s] = 0
            self.status[s] = NOT_TRACKED
            cur_slot[j] = s
        self.next_id[0] += admitted
        self.n_live[0] = int((self.ids >= 0).sum())
        return cur_slot


def fill_pixels(match_index, cur_uv, rows):
    """ftk_nn_fill_pixels_device over a current set padded with zeros to ``rows`` rows: entry t is cur_uv[match_index[t]] where that index
    is valid, and the padded set's row t otherwise."""
    cur_uv = np.asarray(cur_uv, np.float32).reshape(-1, 2)
    padded = np.zeros((max(rows, cur_uv.shape[0]), 2), np.float32)
    padded[:cur_uv.shape[0]] = cur_uv
    out = padded.copy()
    for t in range(len(match_index)):
        if 0 <= int(match_index[t]) < padded.shape[0]:
            out[t] = padded[int(match_index[t])]
    return out
