"""Time the PAPER total order of one whole replay: a persistent-chain DR_DELIVER_PAPER
dr_replay with ids_cap = the mirror's slot count (the a_deliver sequence of the DAG).

Prints one JSON line: the median step time, n_ids, last_ids_form when the library has it,
and with phase timing on ms_emit (the id pass's device time).  The same command runs on an
older library that lacks DR_OPT_DEVICE_IDS (DR_LIB_PATH_EXPT=<its .so>): the option is set
only when the symbol exists, and that run is the host-planned baseline.

usage: python tools/order_timing.py [--config c4] [--steps 20] [--warmup 3] [--timing 0|2]
           [--device-ids 0|1] [--coin const1|seeded|table] [--seed S] [--table 3,1,...]
           [--p-present P --table-absent K] [--verify]

--table-absent K: the table names, for waves 1..K, the lowest source absent in the wave's
first round (no leader vertex: no commit), so the first commit comes late and its pop
delivers everything below it; needs a config with absent sources (--p-present < 1).
--verify: per pop, the count and oracle.digest of its id range against pop_count /
pop_digest, and no id twice.
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from dag_rider_amd import _lib as L  # noqa: E402

# an older library: bind what it has
_has_form = hasattr(C.CDLL(L.LIB_PATH), "dr_last_ids_form")
if not _has_form:
    L.SIGNATURES.pop("dr_last_ids_form", None)

from dag_rider_amd.engine import Engine, Replayer  # noqa: E402
from dag_rider_amd.gen import CONFIGS, generate  # noqa: E402


def absent_table(d, k):
    """For waves 1..k the lowest source with no slot in round 4(w-1)+1."""
    out = []
    for w in range(1, k + 1):
        r = 4 * (w - 1) + 1
        here = np.zeros(d.n + 1, bool)
        here[d.slot_src[d.slot_off[r]:d.slot_off[r + 1]]] = True
        gone = np.nonzero(~here[1:])[0]
        if not len(gone):
            raise SystemExit(f"round {r}: every source present (use --p-present < 1)")
        out.append(int(gone[0]) + 1)
    return out


def verify(res):
    import oracle

    ids = res.ids
    assert len(ids) == int(res.pop_count.sum()), (len(ids), int(res.pop_count.sum()))
    at = 0
    for p, c in enumerate(res.pop_count.tolist()):
        seg = ids[at:at + c]
        assert oracle.digest([(int(r), int(s)) for r, s in seg]) == int(res.pop_digest[p]), f"pop {p}: digest"
        at += c
    key = ids[:, 0].astype(np.int64) << 16 | ids[:, 1].astype(np.int64)
    assert len(np.unique(key)) == len(key), "an id repeats"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timing", type=int, default=0, help="DR_OPT_PHASE_TIMING (2: ms_emit reported)")
    ap.add_argument("--device-ids", type=int, default=1)
    ap.add_argument("--coin", default="const1", choices=["const1", "seeded", "table"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--table", default="")
    ap.add_argument("--table-absent", type=int, default=0)
    ap.add_argument("--p-present", type=float, default=None)
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    cfg = CONFIGS[a.config]
    if a.p_present is not None:
        cfg = dataclasses.replace(cfg, p_present=a.p_present)
    d = generate(cfg, nthreads=16)
    with Engine(cfg.n, cfg.faulty, d.nrounds, 0) as e:
        e.append_packed(d)
        table = None
        if a.table_absent:
            table = absent_table(d, a.table_absent)
        elif a.table:
            table = [int(x) for x in a.table.split(",")]
        if table is not None:
            e.set_leader_coin(L.DR_LEADER_TABLE, table=table)
        elif a.coin == "seeded":
            e.set_leader_coin(L.DR_LEADER_SEEDED, seed=a.seed)
        e.set_phase_timing(a.timing)
        if _has_form:
            e.set_device_ids(bool(a.device_ids))
        slots = e.mirror_stats()["slots"]
        rp = Replayer(e, cfg.nwaves, L.DR_CHAIN_PERSISTENT, L.DR_DELIVER_PAPER, ids_cap=slots)
        for _ in range(a.warmup):
            rp()
        ts, emit = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            rp()
            ts.append((time.perf_counter() - t0) * 1e3)
            emit.append(rp._o.ms_emit)
        res = rp.result()
        out = dict(tool="order_timing", config=cfg.name, n=cfg.n, rounds=d.nrounds - 1, nwaves=cfg.nwaves,
                   p_present=cfg.p_present, coin="table" if table is not None else a.coin,
                   table_absent=a.table_absent, steps=a.steps, step_ms_median=round(statistics.median(ts), 4),
                   step_ms_min=round(min(ts), 4), n_ids=int(rp._o.n_ids), n_push=int(rp._o.n_push),
                   first_commit=int(np.nonzero(res.commit)[0][0]) + 1 if res.commit.any() else 0,
                   first_pop_count=int(res.pop_count[0]) if len(res.pop_count) else 0, slots=slots,
                   build_id=L.build_id())
        if _has_form:
            out["last_ids_form"] = e.last_ids_form()
        if a.timing >= 2:
            out["ms_emit_median"] = round(statistics.median(emit), 4)
        if a.verify:
            verify(res)
            out["verified"] = True
        print(json.dumps(out))


if __name__ == "__main__":
    main()
