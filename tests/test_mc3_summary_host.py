"""diagnostics.rung_trace and diagnostics.replica_flow -- the numpy restatement of csrc/k_mc3_summary.hip that tests/test_gpu_mc3_summary.py
compares the kernels with -- on small hand-built temperature tables with known answers, so that the GPU tests do not compare the code with
itself.  No device."""
import numpy as np
import pytest

from mcmc_date_amd import diagnostics as D

LADDER = np.array([1.0, 0.9, 0.8])


def table(ranks):
    """[n][B] temperature ranks -> beta [n, B]"""
    return LADDER[np.asarray(ranks)]


def test_cold_holder_moves_through_a_group():
    # two groups of three chains; the cold chain of group 0 is 0, then 2, then 1, that of group 1 stays 1
    beta = table([[0, 1, 2, 1, 0, 2],
                  [1, 2, 0, 2, 0, 1],
                  [2, 0, 1, 2, 0, 1]])
    n, B, Q = 3, 6, 4
    x = np.arange(n * B * Q, dtype=np.float64).reshape(n, B, Q)
    tr, holder = D.rung_trace(x, beta, 1.0, 3)
    assert tr.shape == (3, 2, 4) and holder.shape == (3, 2) and holder.dtype == np.int32
    assert np.array_equal(holder, [[0, 1], [2, 1], [1, 1]])
    for k, chains in enumerate([(0, 4), (2, 4), (1, 4)]):
        for g, b in enumerate(chains):
            assert np.array_equal(tr[k, g], x[k, b])
    # the hottest rung: another sequence of the same samples
    tr2, holder2 = D.rung_trace(x, beta, 0.8, 3)
    assert np.array_equal(holder2, [[2, 2], [1, 0], [0, 0]])
    assert np.array_equal(tr2[1, 1], x[1, 3]) and np.array_equal(tr2[2, 0], x[2, 0])
    # one group of six chains would hold two cold chains
    with pytest.raises(ValueError, match="sample 0 of group 0 has 2 chains"):
        D.rung_trace(x, beta, 1.0, 6)


def test_a_row_with_two_matches_or_none_is_refused():
    beta = table([[0, 1, 2], [0, 0, 2], [1, 2, 0]])
    x = np.zeros((3, 3, 2))
    with pytest.raises(ValueError, match="sample 1 of group 0 has 2 chains"):
        D.rung_trace(x, beta, 1.0, 3)
    with pytest.raises(ValueError, match="sample 1 of group 0 has 0 chains"):
        D.rung_trace(x, beta, 0.9, 3)
    D.rung_trace(x, beta, 0.8, 3)                            # (that rung has its one chain everywhere)
    with pytest.raises(ValueError, match="multiple of n_chains"):
        D.rung_trace(x, beta, 1.0, 2)


def test_exactly_one_round_trip():
    # chain 0: cold, down to the hottest rung, back to cold (one passage), half way down again; chain 1 starts hot: reaching the cold
    # rung arms it, the passage back to the hottest rung and half way up is not a completed one; chain 2 never leaves the middle
    ranks = np.array([[0, 2, 1],
                      [1, 2, 1],
                      [2, 0, 1],
                      [2, 0, 1],
                      [1, 2, 1],
                      [0, 2, 1],
                      [1, 2, 1],
                      [2, 1, 1]])
    ranks[:, 2] = 1
    visits, trips = D.replica_flow(table(ranks), LADDER)
    assert visits.dtype == np.int64 and trips.dtype == np.int64
    assert np.array_equal(trips, [1, 0, 0])
    assert np.array_equal(visits, [[2, 3, 3], [2, 1, 5], [0, 8, 0]])
    assert np.array_equal(visits.sum(axis=1), [8, 8, 8])


def test_two_passages_and_a_temperature_off_the_ladder():
    ranks = np.array([[0], [2], [0], [1], [2], [2], [0], [2]])
    beta = table(ranks)
    visits, trips = D.replica_flow(beta, LADDER)
    assert trips[0] == 2 and np.array_equal(visits[0], [3, 1, 4])
    beta[3, 0] = 0.85                                        # counts nowhere and moves nothing
    visits, trips = D.replica_flow(beta, LADDER)
    assert trips[0] == 2 and np.array_equal(visits[0], [3, 0, 4]) and visits.sum() == 7
    # a ladder of two rungs: the hottest is rung 1; the chain that starts hot is armed one sample later and needs one more to come back
    v2, t2 = D.replica_flow(np.array([[1.0, 0.5], [0.5, 1.0], [1.0, 0.5], [0.5, 1.0], [1.0, 0.5]]), [1.0, 0.5])
    assert np.array_equal(t2, [2, 1]) and np.array_equal(v2, [[3, 2], [2, 3]])


def test_rung_trace_against_a_plain_loop():
    rng = np.random.default_rng(3)
    n, G, C, Q = 17, 5, 4, 7
    ladder = 0.97 ** np.arange(C)
    ranks = np.stack([np.concatenate([rng.permutation(C) for _ in range(G)]) for _ in range(n)])
    beta = ladder[ranks]
    x = rng.standard_normal((n, G * C, Q))
    for r in range(C):
        tr, holder = D.rung_trace(x, beta, ladder[r], C)
        for k in range(n):
            for g in range(G):
                h = int(np.nonzero(ranks[k, g * C:(g + 1) * C] == r)[0][0])
                assert holder[k, g] == h and np.array_equal(tr[k, g], x[k, g * C + h])
    visits, _ = D.replica_flow(beta, ladder)
    assert np.array_equal(visits.sum(axis=1), np.full(G * C, n))
    assert np.array_equal(visits.sum(axis=0) , np.full(C, n * G))
