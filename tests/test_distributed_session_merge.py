"""The gathered session balance over two gloo ranks (needs no GPU): each rank's host handle holds alternate segments' additions, rank 0
also the verifier's side; driver.exchange_session_classes -- the step driver.prove_elf_sharded(check_session=True) runs -- must leave
both ranks with the message of one handle that had every addition, for a balanced set and for one with an altered hand-over value."""
import os
import sys

import torch.multiprocessing as mp

from conftest import ROOT
from test_distributed import _free_port


def _worker(rank, world, port, broken, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import hyperfridge_r0_amd as r0
    from hyperfridge_r0_amd import driver
    from test_session_merge import additions, feed
    env = driver.DistEnv(backend="gloo")
    blob, adds = additions(broken=broken)
    segments, outside = [a for a in adds if a[0] == "segment"], [a for a in adds if a[0] == "outside"]
    sb = feed(r0.SessionBalance(blob), segments[rank::world] + (outside if rank == 0 else []))
    own = sb.message()
    timings = {}
    text = driver.exchange_session_classes(env, sb, timings)
    out.put((rank, own, text, sb.export().tobytes(), timings["exported_bytes"], sb.stats()[0]))
    env.close()


def _two_ranks(broken):
    world = 2
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, broken, out)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted(out.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return results


def _single(broken):
    import hyperfridge_r0_amd as r0
    from test_session_merge import additions, feed
    blob, adds = additions(broken=broken)
    return feed(r0.SessionBalance(blob), adds)


def test_two_ranks_agree_on_a_balanced_session():
    single = _single(False)
    (_, own0, text0, export0, bytes0, tuples0), (_, own1, text1, export1, bytes1, tuples1) = _two_ranks(False)
    assert own0 is not None and own1 is not None            # each rank alone sees hand-overs whose other side is elsewhere
    assert text0 is None and text1 is None and single.message() is None
    assert export0 == export1 == single.export().tobytes() and tuples0 == tuples1 == single.stats()[0]
    assert bytes0 % 64 == 0 and bytes1 % 64 == 0 and bytes0 != bytes1       # lists of different lengths: the shorter one travelled padded


def test_two_ranks_name_the_same_altered_hand_over():
    single = _single(True)
    (_, _, text0, export0, _, _), (_, _, text1, export1, _, _) = _two_ranks(True)
    assert text0 == text1 == single.message() and text0.startswith("session fraction 4 does not balance: net 1 over 1 tuples, first in source 1 at row ")
    assert text0.endswith("2 classes in all") and export0 == export1 == single.export().tobytes()
