"""The PAPER total order (DR_DELIVER_PAPER ids: every vertex once, by the first pop whose cone
holds it -- Alg. 3 line 54, the a_deliver sequence) written by the device-planned replay's id
pass (DR_OPT_DEVICE_IDS, replay_plan.hpp k_paper_ids), against the CPU oracles, bit-exact:
ids, pop_count, pop_digest, pop_edges, pushes and commits.

The id pass is under test only where last_ids_form() == 1 is asserted: a replay that fell
back to the host-planned path would pass the comparison without running it.  Weak edges stay
at most 11 rounds deep so the memo (round summaries + canonical cone) applies."""
import ctypes as C

import numpy as np
import pytest

import oracle
from dag_rider_amd import _lib as L
from dag_rider_amd.dag import PackedDag, flatten_lists
from dag_rider_amd.engine import Engine, _replay_out
from dagutil import figure1, random_dag, with_irregular_edges, with_repeated_ids

pytestmark = pytest.mark.gpu

CHAINS = (L.DR_CHAIN_LITERAL, L.DR_CHAIN_PERSISTENT)
PAPER, REF = L.DR_DELIVER_PAPER, L.DR_DELIVER_REF
CAP = 1 << 16


def _same(got, want):
    assert got.commit.tolist() == want.commit.tolist()
    assert got.vcount.tolist() == want.vcount.tolist()
    assert got.push_off.tolist() == want.push_off.tolist()
    assert got.push_wave.tolist() == want.push_wave.tolist()
    assert got.pop_count.tolist() == want.pop_count.tolist()
    assert got.pop_digest.tolist() == want.pop_digest.tolist()
    assert got.pop_edges.tolist() == want.pop_edges.tolist()
    assert (got.commit_edges, got.deliver_edges) == (want.commit_edges, want.deliver_edges)
    assert got.ids.tolist() == want.ids.tolist()


def _sparse_dag(rng, n, R, depth=6):
    """random_dag with a strong degree that does not grow with n (the builder is a Python
    loop per edge) yet leaves most waves committing: ~10 strong edges a vertex."""
    return random_dag(rng, n, R, p_present=0.9, p_s=min(0.6, 10.0 / n), p_w=0.5, max_depth=depth)


# ----------------------------------------------------------------------------- 1. word counts
@pytest.mark.parametrize("case,n", list(enumerate([4, 65, 130, 257, 513, 1100])))
def test_word_counts(gpu_device, case, n):
    """WS = 1, 2, 4, 8, 16, 32; both chain modes (the literal chains pop a leader again and
    again: pops that deliver nothing, pops with equal positions); the DAG appended in two
    chunks; every other case with every launch grouping (DR_OPT_FUSE 63)."""
    rng = np.random.default_rng(4100 + n)
    R = 24
    d = _sparse_dag(rng, n, R, depth=int(rng.integers(2, 12)))
    f = 0 if n < 4 else int(rng.integers(0, 2))
    nw = R // 4
    ref = oracle.LDag(packed=d) if n <= 16 else oracle.PDag(d)
    with Engine(n, f, R + 1, gpu_device) as e:
        if case % 2:
            e.set_fuse(63)
        cut = int(rng.integers(1, R + 1))
        e.append_packed(d, 0, cut)
        e.append_packed(d, cut, d.nrounds)
        delivered = 0
        for cm in CHAINS:
            want = ref.replay(f, nw, cm, PAPER, ids_cap=CAP)
            assert want.rc == 0
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want)
            delivered += len(got.ids)
        assert delivered > 0  # the case delivers something to order


# ------------------------------------------------------------ 2. repeated ids and ghost slots
@pytest.mark.parametrize("n,R", [(10, 20), (100, 12)])
def test_repeated_ids(gpu_device, n, R):
    """PAPER delivers a repeated id once, at its first slot (slot_rep drops the later ones)."""
    rng = np.random.default_rng(4200 + n)
    base = random_dag(rng, n, R, p_present=0.9, p_s=min(0.7, 12.0 / n), p_w=0.4, max_depth=6).to_lists()
    dag = with_repeated_ids(rng, base, p_dup=0.35)
    f = 1
    nw = R // 4
    ld = oracle.LDag(arrays=flatten_lists(dag))
    with Engine(n, f, R + 1, gpu_device) as e:
        e.append_lists(dag)
        assert e.mirror_stats()["slots"] > sum(len({v.id for v in r}) for r in dag)  # ids do repeat
        for cm in CHAINS:
            want = ld.replay(f, nw, cm, PAPER, ids_cap=CAP)
            assert want.rc == 0
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want)
            assert len(got.ids) > 0 and len({tuple(x) for x in got.ids.tolist()}) == len(got.ids)


def test_figure1_ghost_slot(gpu_device):
    g, dag = figure1()
    R = len(dag) - 1
    ld = oracle.LDag(arrays=flatten_lists(dag))
    with Engine(g["n"], g["faulty"], R + 1, gpu_device) as e:
        e.append_lists(dag)
        for cm in CHAINS:
            want = ld.replay(g["faulty"], R // 4, cm, PAPER, ids_cap=CAP)
            assert want.rc == 0
            got = e.replay(R // 4, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want)


# ------------------------------------------------- 3. late first commit, long canonical range
def _late_dag(rng, n, R, late):
    """Sources 1..n-1 present with probability 0.9 (source 1 always in a wave's first round),
    source n absent in the first round of waves 1..late; dense strong edges, a few weak ones."""
    assert n <= 64
    NR = R + 1
    pres = rng.random((NR, n)) < 0.9
    pres[0] = True
    first = np.arange(1, NR, 4)  # rounds 4(w-1)+1
    pres[first, 0] = True
    pres[first[:late], n - 1] = False
    hit = (rng.random((NR, n, n)) < 0.8) & pres[:, :, None]
    hit[1:] &= pres[:-1, None, :]
    hit[0] = False
    strong = (hit.astype(np.uint64) << np.arange(n, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).reshape(-1)
    slot_off, slot_src = [0], []
    for r in range(NR):
        s = (np.nonzero(pres[r])[0] + 1).tolist()
        rng.shuffle(s)
        slot_src += s
        slot_off.append(len(slot_src))
    weak_off, weak_tgt = [0], []
    for r in range(NR):
        for s in range(n):
            if pres[r, s] and r >= 3 and rng.random() < 0.2:
                weak_tgt.append(((r - 2 - int(rng.integers(0, min(r - 2, 5)))) << 11) | int(rng.integers(0, n)))
            weak_off.append(len(weak_tgt))
    return PackedDag(n, NR, np.asarray(slot_off, np.uint32), np.asarray(slot_src, np.uint16), strong,
                     np.asarray(weak_off, np.uint32), np.asarray(weak_tgt, np.uint32))


def test_late_first_commit(gpu_device):
    """No wave up to 580 has a leader vertex, so the first pop delivers well over 512 rounds
    at once: k_paper_emit's binary search for the range's first round, and a range written by
    many workgroups of the id pass."""
    n, R, late = 8, 2400, 580
    rng = np.random.default_rng(4300)
    d = _late_dag(rng, n, R, late)
    f, nw = 2, R // 4
    leaders = [n] * late
    pd = oracle.PDag(d, leaders=leaders)
    # the literal oracle's BFS per pop is quadratic in the DAG's length (minutes at R = 2400):
    # it vouches for the bitset oracle under the same coin on the same shape at R = 120
    ds = _late_dag(np.random.default_rng(4301), n, 120, 25)
    for cm in CHAINS:
        a = oracle.LDag(packed=ds, leaders=[n] * 25).replay(f, 30, cm, PAPER, ids_cap=CAP)
        b = oracle.PDag(ds, leaders=[n] * 25).replay(f, 30, cm, PAPER, ids_cap=CAP)
        assert a.rc == b.rc == 0 and int(np.nonzero(b.commit)[0][0]) + 1 > 25
        assert a.ids.tolist() == b.ids.tolist() and a.pop_digest.tolist() == b.pop_digest.tolist()
    with Engine(n, f, R + 1, gpu_device) as e:
        e.append_packed(d)
        e.set_leader_coin(L.DR_LEADER_TABLE, table=leaders)
        for cm in CHAINS:
            want = pd.replay(f, nw, cm, PAPER, ids_cap=CAP)
            assert want.rc == 0
            # the shape, by the oracle: nothing commits up to wave 580, the first pop takes it all
            first = int(np.nonzero(want.commit)[0][0]) + 1
            assert first > late and int(want.pop_count[0]) > 512 * n // 2
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want)
            assert got.chain_edges == want.chain_edges


# ------------------------------------------------------------------------------ 4. truncation
@pytest.fixture(scope="module")
def dag130():
    rng = np.random.default_rng(4400)
    n, R = 130, 24
    d = _sparse_dag(rng, n, R)
    return n, R, 1, d, oracle.PDag(d)


def test_truncation(gpu_device, dag130):
    """n_ids is the whole stream's length however small ids_cap is; nothing is written at or
    beyond ids_cap; the call returns DR_OK."""
    n, R, f, d, ref = dag130
    nw = R // 4
    cm = L.DR_CHAIN_PERSISTENT
    want = ref.replay(f, nw, cm, PAPER, ids_cap=CAP)
    total = len(want.ids)
    assert total > 4
    with Engine(n, f, R + 1, gpu_device) as e:
        e.append_packed(d)
        for cap in (1, total // 2):
            o, keep = _replay_out(nw, cm, cap)
            ids = np.full(2 * (total + 8), -7, np.int32)
            o.ids = ids.ctypes.data
            rc = e._L.dr_replay(e._h, nw, cm, PAPER, C.byref(o))
            assert rc == L.DR_OK
            assert e.last_ids_form() == 1
            assert o.n_ids == total
            assert ids[:2 * cap].reshape(-1, 2).tolist() == want.ids[:cap].tolist()
            assert (ids[2 * cap:] == -7).all()
            assert keep["pc"][:o.n_push].tolist() == want.pop_count.tolist()
            assert keep["pdg"][:o.n_push].tolist() == want.pop_digest.tolist()


# -------------------------------------------------------------------- 5. option and fallbacks
def test_option_and_fallbacks(gpu_device, dag130):
    n, R, f, d, ref = dag130
    nw = R // 4
    with Engine(n, f, R + 1, gpu_device) as e:
        e.append_packed(d)
        assert e.last_ids_form() == -1
        e.replay(nw, CHAINS[0], PAPER)
        e.replay(nw, CHAINS[0], REF)
        assert e.last_ids_form() == -1  # no replay asked for ids yet
        for cm in CHAINS:
            want = ref.replay(f, nw, cm, PAPER, ids_cap=CAP)
            want_ref = ref.replay(f, nw, cm, REF, ids_cap=1 << 20)
            assert want.rc == 0 and want_ref.rc == 0
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want)
            e.replay(nw, cm, PAPER)
            e.replay(nw, cm, REF)
            assert e.last_ids_form() == 1  # replays without ids leave it
            e.set_device_ids(False)
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 0
            _same(got, want)
            e.set_device_ids(True)
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            got = e.replay(nw, cm, REF, ids_cap=1 << 20)  # REF ids: host-planned on purpose
            assert e.last_ids_form() == 0
            _same(got, want_ref)
            e.set_memo(False)
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 0
            _same(got, want)
            e.set_memo(True)
            e.set_device_plan(False)
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 0
            _same(got, want)
            e.set_device_plan(True)
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want)


def test_upward_weak_edge_falls_back(gpu_device):
    """A DAG with weak edges to the same or a later round (App. A Q8) takes the general sweep."""
    rng = np.random.default_rng(4500)
    n, R, f = 7, 16, 1
    base = random_dag(rng, n, R, p_present=0.9, p_s=0.7, p_w=0.3, max_depth=5).to_lists()
    dag = with_irregular_edges(rng, base, p_irr=0.1, up=True)
    ld = oracle.LDag(arrays=flatten_lists(dag))
    with Engine(n, f, R + 1, gpu_device) as e:
        e.append_lists(dag)
        assert e.exception_stats()["upward"] >= 1
        for cm in CHAINS:
            want = ld.replay(f, R // 4, cm, PAPER, ids_cap=CAP)
            assert want.rc == 0
            got = e.replay(R // 4, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 0
            _same(got, want)


# ------------------------------------------------------- 6. replay twice, and after an append
def test_replay_twice_and_after_append(gpu_device):
    rng = np.random.default_rng(4600)
    n, R, f = 257, 40, 1
    d = _sparse_dag(rng, n, R)
    ref = oracle.PDag(d)
    nw1, nw2 = 3, R // 4
    cm = L.DR_CHAIN_PERSISTENT
    with Engine(n, f, R + 1, gpu_device) as e:
        e.append_packed(d, 0, 4 * nw1 + 1)
        want1 = ref.replay(f, nw1, cm, PAPER, ids_cap=CAP)  # the waves read rounds <= 4 nw1 only
        for _ in range(2):
            got = e.replay(nw1, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want1)
        e.append_packed(d, 4 * nw1 + 1, d.nrounds)
        want2 = ref.replay(f, nw2, cm, PAPER, ids_cap=CAP)
        assert len(want2.ids) > 2 * len(want1.ids) > 0  # the id buffer has to grow
        for _ in range(2):
            got = e.replay(nw2, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1
            _same(got, want2)


# ---------------------------------------------------------------- 7. DR_OPT_REPLAY_GRAPH + ids
def test_replay_graph_with_ids(gpu_device, dag130):
    """A replay that requests ids launches kernel by kernel (its buffers are no part of the
    graph's key); a replay without ids after it may capture as before."""
    n, R, f, d, ref = dag130
    nw = R // 4
    cm = L.DR_CHAIN_PERSISTENT
    want = ref.replay(f, nw, cm, PAPER, ids_cap=CAP)
    with Engine(n, f, R + 1, gpu_device) as e:
        e.append_packed(d)
        e.set_phase_timing(0)
        e.set_replay_graph(True)
        for _ in range(3):
            got = e.replay(nw, cm, PAPER, ids_cap=CAP)
            assert e.last_ids_form() == 1 and e.replay_graph_state() == 0
            _same(got, want)
        states = []
        for _ in range(3):
            got = e.replay(nw, cm, PAPER)
            states.append(e.replay_graph_state())
            assert got.pop_digest.tolist() == want.pop_digest.tolist()
            assert got.pop_count.tolist() == want.pop_count.tolist()
        assert states[-1] == 1  # captured and launched
        got = e.replay(nw, cm, PAPER, ids_cap=CAP)
        assert e.last_ids_form() == 1 and e.replay_graph_state() == 0
        _same(got, want)
