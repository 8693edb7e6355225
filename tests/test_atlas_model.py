"""tests/atlas_model.py checked alone (CPU): the derived tables' invariants, the river equity bits, a 3-bucket chain computed by hand,
the tie rule of the neighbours and the draw-to-position rule."""
import numpy as np

import atlas_model as AM
import oracle_deuce as od

F = np.float32


def flop_model(K=7):
    obs = od.isomorphisms("flop", 0, 8)
    labels = ((obs.astype(np.uint64) * np.uint64(2654435761)) >> np.uint64(20)) % np.uint64(K)
    river = AM.Atlas(3, [], [], 101)
    turn = AM.Atlas(2, [], [], 3, np.zeros((3, 101), np.uint32), np.zeros(3, np.uint64), None, None, river)
    fut = np.arange(K * 3, dtype=np.uint32).reshape(K, 3)
    tri = (np.arange(K * (K - 1) // 2) % 3 / 8.0).astype(F)
    return obs, labels, AM.Atlas(1, obs, labels, K, fut, fut.sum(axis=1).astype(np.uint64), tri, None, turn)


def test_positions_are_a_permutation_per_bucket_ascending_in_obs():
    obs, labels, m = flop_model()
    assert int((np.diff(obs) < 0).sum()) == 533  # the table's order is not the BIGINT order
    assert int(m.population.sum()) == obs.size == 6_212 and m.offset[-1] == obs.size
    for k in range(m.K):
        rows = np.flatnonzero(labels == k)
        assert sorted(m.position[rows].tolist()) == list(range(int(m.population[k])))
        by_pos = rows[np.argsort(m.position[rows])]
        assert (np.diff(obs[by_pos]) > 0).all()
        assert np.array_equal(m.members[m.offset[k]:m.offset[k + 1]], by_pos)
    # the same through numpy's own sort
    assert np.array_equal(m.members, np.lexsort((obs, labels)))


def test_river_equity_bits_under_both_readings_of_real_over_100():
    for k in range(101):
        assert AM.river_equity(k).tobytes() == F(float(k) / 100.0).tobytes() == (F(k) / F(100)).tobytes()
    assert np.array_equal(AM.Atlas(3, [], [], 101).equity, (np.arange(101) / 100.0).astype(F))


def test_equity_of_a_three_bucket_chain_by_hand():
    river = AM.Atlas(3, [], [], 101)
    # turn bucket 0 -> river bins 100 (3 of 4) and 0 (1 of 4); bucket 1 -> bins 50 and 20 evenly; bucket 2 has no rows
    fut = np.zeros((3, 101), np.uint32)
    fut[0, 100], fut[0, 0] = 3, 1
    fut[1, 50], fut[1, 20] = 2, 2
    turn = AM.Atlas(2, [], [], 3, fut, np.array([4, 4, 0], np.uint64), None, None, river)
    assert turn.rows[0] == [(100, F(0.75)), (0, F(0.25))] and turn.rows[1] == [(20, F(0.5)), (50, F(0.5))] and turn.rows[2] == []
    assert turn.equity[0] == F(0.75) and turn.fold[0] == F(0.75)  # 0.75 * 1.0 + 0.25 * 0.0 over 1.0
    e1 = F(F(F(0.5) * F(0.2)) + F(F(0.5) * F(0.5)))  # bin 20 first: equal densities keep the bin order
    assert turn.equity[1].tobytes() == F(e1 / F(1.0)).tobytes() and turn.equity[2] == 0 and turn.fold[2] == 0
    # flop bucket 0 -> turn buckets 0, 1, 2 with counts 1, 2, 1: dx 0.5 (bucket 1) first, then 0.25 (bucket 0), 0.25 (bucket 2)
    flop = AM.Atlas(1, [], [], 1, np.array([[1, 2, 1]], np.uint32), np.array([4], np.uint64), None, None, turn)
    num = F(F(F(0.5) * turn.equity[1]) + F(F(0.25) * F(0.75)))
    num = F(num + F(F(0.25) * F(0.0)))
    assert flop.rows[0] == [(1, F(0.5)), (0, F(0.25)), (2, F(0.25))]
    assert flop.fold[0].tobytes() == num.tobytes() and flop.equity[0].tobytes() == F(num / F(1.0)).tobytes()


def test_ties_go_to_the_smaller_index_both_ways():
    K = 5
    tri = np.zeros(K * (K - 1) // 2, F)
    for c, d in ((0, 0.5), (1, 0.25), (3, 0.5), (4, 0.25)):
        tri[AM.pair(2, c)] = d
    river = AM.Atlas(3, [], [], 2)
    m = AM.Atlas(2, [], [], K, np.zeros((K, 2), np.uint32), np.zeros(K, np.uint64), tri, None, river)
    near, _ = m.neighbors([2], 4)
    far, _ = m.neighbors([2], 4, farthest=True)
    assert (near["abs"][0] & 0xFF).tolist() == [1, 4, 0, 3] and (far["abs"][0] & 0xFF).tolist() == [0, 3, 1, 4]
    assert near["distance"][0].tolist() == [0.25, 0.25, 0.5, 0.5]
    assert m.distance([2, 2, 7], [2, 0, 0]).tolist()[:2] == [0.0, 0.5] and np.isnan(m.distance([7], [0])[0])


def test_draw_to_position():
    top = (1 << 64) - 1
    assert AM.draw_index(0, 1) == AM.draw_index(top, 1) == AM.draw_index(1 << 63, 1) == 0
    for population in (2, 3, 1000, 6_212, 123_156_254, 1 << 27):
        assert AM.draw_index(0, population) == 0 and AM.draw_index(top, population) == population - 1
        assert AM.draw_index(1 << 63, population) == population // 2
    _, _, m = flop_model()
    s, st = m.pick([0, 0, 6, 7], [0, top, 1 << 63, 0])
    assert st.tolist() == [AM.OK, AM.OK, AM.OK, AM.RANGE]
    assert s["position"].tolist() == [0, m.population[0] - 1, m.population[6] // 2, 0]
    assert s["obs"][0] == min(m.obs[i] for i in m.bucket[0]) and s["obs"][1] == max(m.obs[i] for i in m.bucket[0])


def test_describe_and_windows_on_the_flop_prefix():
    obs, labels, m = flop_model()
    s, st = m.describe([int(obs[5]), 0, int(obs[5]) >> 8], [int(labels[5]), 0, 0])
    assert st.tolist() == [AM.SAME, AM.MISS, AM.MISS] and s["abs"][0] == (1 << 8 | int(labels[5])) and s["distance"][0] == 0
    assert s["density"][0] == F(m.population[labels[5]]) / F(25_989_600)
    out, got = m.window([0, 0], [int(m.population[0]) - 2, int(m.population[0])], 6)
    assert got.tolist() == [2, 0] and (out[0, 2:] == 0).all() and out[0, 0] < out[0, 1]
