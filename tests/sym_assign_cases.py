"""Known answers for the assign step of the deterministic sym schedule (ggnn_set_build_hooks,
serial_sym = 2; oracle `orc_sym_assign`, kernel `sym_assign_kernel`), shared by the CPU tests
(tests/test_oracle_restatements.py) and the GPU tests (tests/test_gpu_deterministic_sym.py).

The step, from include/ggnn_c.h and oracle/ggnn_oracle.hpp: request rows are visited in ascending
(point n, local neighbour j) order.  The candidates c of a row count up to the first -1 or id
>= Nlayer.  If n is among sym_buffer[c][0 .. min(sym_atomic[c], KF)) the row is done and nothing
changes; else pos = sym_atomic[c]++, and if pos < KF then sym_buffer[c][pos] = n and the row is
done, else the next candidate is asked.

Every case is (name, KBuild, requests [N, KL, KF], atomic before, buffer before, atomic after,
buffer after); KF = KBuild // 2, KL = KBuild - KF.  The expected arrays of CASES are written out by
hand; the walk that gives them is in the comment above each.  row_count_cases() derives its
expectation from a closed formula explained there."""
import numpy as np

E = -1


def _case(name, K, requests, atomic0, buffer0, atomic1, buffer1):
    KF = K // 2
    KL = K - KF
    req = np.array(requests, np.int32)
    N = req.shape[0]
    assert req.shape == (N, KL, KF), (name, req.shape)
    out = [name, K, req]
    for a, b in ((atomic0, buffer0), (atomic1, buffer1)):
        out.append(np.zeros(N, np.uint32) if a is None else np.array(a, np.uint32))
        out.append(np.full((N, KF), E, np.int32) if b is None else np.array(b, np.int32))
        assert out[-2].shape == (N,) and out[-1].shape == (N, KF), name
    return tuple(out)


NONE2 = [E, E]
NONE3 = [E, E, E]

CASES = [
    # K = 4: KF = 2 slots per target, KL = 2 searches per point.  Points 1..4 all ask target 0
    # first.  1 and 2 take its two slots.  3 finds it full (counter 2 -> 3) and goes on to 4.
    # 4 finds it full (3 -> 4) and goes on to 1.  The counter of 0 ends at 4 > KF.
    _case("overflow_moves_later_rows_to_their_second_candidate", 4,
          [[NONE2, NONE2],
           [[0, 2], NONE2],
           [[0, 3], NONE2],
           [[0, 4], NONE2],
           [[0, 1], NONE2]],
          None, None,
          [4, 1, 0, 0, 1],
          [[1, 2], [4, E], NONE2, NONE2, [3, E]]),
    # Point 1 asks target 0 from both of its searches: the second row finds 1 in slot 0 of
    # target 0, is done, and does not bump the counter.  Point 2 then takes slot 1 of target 0,
    # and with its second search slot 0 of target 1.
    _case("same_point_same_target_twice_holds_one_slot", 4,
          [[NONE2, NONE2],
           [[0, 2], [0, 2]],
           [[0, E], [1, E]]],
          None, None,
          [2, 1, 0],
          [[1, 2], [2, E], NONE2]),
    # Given state: target 0 is full with {4, 5} and its counter stands at 5 > KF; target 1 holds
    # {3}; target 2 has counter 1, slot 0 = 5, and a stale 3 behind the counter.
    # (3, 0): target 0, slots {4, 5}: not held (row 1 = [3, E] lies right behind row 0 in memory:
    #         a scan of 5 entries would find a 3 there), counter 5 -> 6, full; target 1 holds 3:
    #         done, counter of 1 untouched.
    # (3, 1): target 2, valid slots {5}: the stale 3 does not count, pos = 1 < KF, slot 1 = 3,
    #         counter 1 -> 2.
    # (4, 0): target 0 holds 4 (counter 6 > KF): done, nothing changes.
    _case("held_only_within_min_counter_KF", 4,
          [[NONE2, NONE2],
           [NONE2, NONE2],
           [NONE2, NONE2],
           [[0, 1], [2, E]],
           [[0, E], NONE2],
           [NONE2, NONE2]],
          [5, 1, 1, 0, 0, 0],
          [[4, 5], [3, E], [5, 3], NONE2, NONE2, NONE2],
          [6, 1, 2, 0, 0, 0],
          [[4, 5], [3, E], [5, 3], NONE2, NONE2, NONE2]),
    # K = 6: KF = 3, KL = 3, five points.
    # (0, 0): all -1.  (0, 1): first candidate -1, the later 2 and 3 are never asked.
    # (0, 2): target 1 slot 0 = 0.
    # (2, 0): target 1 slot 1 = 2.  (2, 1): 5 >= Nlayer ends the row before 1 and 3.
    # (2, 2): 2 holds a slot at 1: done.
    # (3, 0): target 1 slot 2 = 3, counter 3.
    # (4, 0): target 1 full, 3 -> 4; 5 >= Nlayer ends the row, 0 is never asked.
    # (4, 1): target 1 full, 4 -> 5; -1 ends the row.
    # (4, 2): target 1 full, 5 -> 6; target 0 slot 0 = 4.
    _case("empty_rows_skipped_rows_and_ids_outside_the_layer", 6,
          [[NONE3, [E, 2, 3], [1, 7, 2]],
           [NONE3, NONE3, NONE3],
           [[1, 9, 3], [5, 1, 3], [1, 3, E]],
           [[1, E, E], NONE3, NONE3],
           [[1, 5, 0], [1, E, 0], [1, 0, 2]]],
          None, None,
          [1, 6, 0, 0, 0],
          [[4, E, E], [0, 2, 3], NONE3, NONE3, NONE3]),
]


def row_count_cases():
    """Nlayer * KL = 63, 64, 65 and 129 request rows (the kernel reads 64 rows at a time).  Row
    (n, j) asks the one target (n + 1 + j) % N; N > KL + 1, so no point asks itself or one target
    twice and nothing is ever held.  Target c is therefore asked by the KL points (c - 1 - j) % N,
    each once, in ascending order of the asking point: its counter ends at KL and its KF slots
    hold the KF smallest of those ids, ascending.  The last row of the table, (N - 1, KL - 1), is
    one of the KL requests of target KL - 1, and every lane of a block of 64 carries a request."""
    out = []
    for K, N in ((6, 21), (4, 32), (8, 16), (10, 13), (9, 13), (6, 43), (5, 43)):
        KF = K // 2
        KL = K - KF
        assert N > KL + 1
        req = np.full((N, KL, KF), E, np.int32)
        for n in range(N):
            for j in range(KL):
                req[n, j, 0] = (n + 1 + j) % N
        atomic = np.full(N, KL, np.uint32)
        buffer = np.array([sorted((c - 1 - j) % N for j in range(KL))[:KF] for c in range(N)],
                          np.int32)
        out.append((f"rows_{N * KL}_K{K}", K, req, np.zeros(N, np.uint32),
                    np.full((N, KF), E, np.int32), atomic, buffer))
    assert sorted({c[2].shape[0] * c[2].shape[1] for c in out}) == [63, 64, 65, 129]
    return out


def all_cases():
    return CASES + row_count_cases()


def contention_table(N, K, targets, seed):
    """every row of N points asks KF distinct targets out of `targets`, so that most rows pass
    several full targets before they find a slot (or none)"""
    KF = K // 2
    KL = K - KF
    r = np.random.default_rng(seed)
    pool = r.choice(N, targets, replace=False)
    pick = np.argsort(r.random((N * KL, targets)), axis=1)[:, :KF]
    return pool[pick].reshape(N, KL, KF).astype(np.int32)
