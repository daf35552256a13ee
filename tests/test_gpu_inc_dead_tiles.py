"""GPU tests (run with -m gpu on an MI355X) of the rank-k update (csrc/k_inc.hip, inc_post) at the live widths a0 = 3 + 2 L0 where
the last column pair of its tile pass ("B3") holds ONE live tile and a tile of pad columns (a0 - 32 (pairs - 1) <= 16), and of its
k x k system assembled by all threads ("B2", narrow and wide), on the worlds of tests/step_cases.py.  (Leaving the pad tile alone
was measured and not kept - profiles/rank_k_dead_tiles_ab.txt; the cases hold for either form of the pass.)

The short script (7 poses, the dense kernels): rings 16, 17, 32, 33 (panel in LDS) and 48, 52, 63, 64 (panel in place) have such a
pad tile, rings 8, 9, 24, 25 do not; the gate steps of 17 + 12, 33 + 13 and 52 + 12 put the new landmarks' columns into it.  Ring 8
takes the narrow assembly, every other ring the wide one (ring 17: a wide batch, then a narrow one).  Tolerances: those of
tests/test_gpu_step_edges.py for the same quantities (estimates 1e-9, information blocks rtol 1e-7 / atol 1e-6 between engines,
compare_state against the oracle); A/Bs of kernel form and repeated runs bit-equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lazy_panel_cases as LP  # noqa: E402
import step_cases as S  # noqa: E402
import test_gpu_lazy_panel as LZ  # noqa: E402
import test_gpu_step_edges as E  # noqa: E402
from test_gpu_belief import compare_state  # noqa: E402

RINGS = {"small": (8, 9, 16, 17, 24, 25, 32, 33), "large": (48, 52, 63, 64)}


@pytest.mark.parametrize("wname", ["small", "large"])
def test_short_script_at_pad_tiles(wname, monkeypatch):
    """Two incremental engines, an engine created under DRLGX_INCREMENTAL=0 and the oracle side by side, the environments stepped
    one at a time so that inc_stats says which path served which ring: after every step estimates, information blocks and marginals
    against the oracle and the full solve, and the two incremental runs bit for bit."""
    world, forms = S.WORLDS[wname](), S.FORMS[wname]["short"]
    sims = world.make_sims()
    eng, again = E._engine(world), E._engine(world)
    monkeypatch.setenv("DRLGX_INCREMENTAL", "0")
    ref = E._engine(world)
    monkeypatch.delenv("DRLGX_INCREMENTAL")
    assert ref.inc_stats() == (-1, -1) and eng.inc_stats() == (0, world.n)
    counts = world.expected_counts(S.SHORT)
    served = set()
    for s, kind in enumerate(S.SHORT):
        acts = world.actions(sims, kind, s)
        for e, (size, _) in enumerate(world.rings):
            want = S.expected_path(counts[s + 1][e], s + 2, S.relinearises(sims[e])[0])
            if (size, s) in forms:
                assert want == "inc", (size, s)
            b0 = eng.inc_stats()
            E._step([eng, again, ref], acts, only=e)
            b1 = eng.inc_stats()
            got = {(1, 0): "inc", (0, 1): "full"}.get((b1[0] - b0[0], b1[1] - b0[1]))
            assert got == want, "%s step %d ring %d %s: served by %s, expected %s" % (wname, s, size, counts[s + 1][e], got, want)
            if got == "inc":
                served.add((size, s))
        for sim, a in zip(sims, acts):
            sim.simulate(a)
        assert eng.status() == 0 and again.status() == 0 and ref.status() == 0
        for i, sim in enumerate(sims):
            name = "%s step %d ring %d" % (wname, s, world.rings[i][0])
            compare_state(eng, i, sim, "incremental, " + name, check_vm=True)
            compare_state(ref, i, sim, "full solve, " + name, check_vm=True)
            E._compare_engines(eng, ref, i, name)
            E._assert_bits(E._dump(eng, i) + tuple(eng.cov_traces(i)), E._dump(again, i) + tuple(again.cov_traces(i)), "two runs, " + name)
    # no case fell to the full solve: every (ring, step) of the table, and every jiggle step of every ring listed above
    assert set(forms) <= served
    assert {(r, s) for r in RINGS[wname] for s in (0, 1, 3, 5)} <= served
    for e in (eng, again, ref):
        e.close()


@pytest.mark.parametrize("which,ring,form", [("inplace", 48, "two-walk wide"), ("small", 16, "lds wide")])
def test_step_behind_a_lazy_restore(which, ring, form):
    """The update that reads its panel from the snapshot (the restore left it there), ring 48 in place and ring 16 in LDS - a pad
    tile either way: bit for bit the step of an engine created under DRLGX_RESTORE_EAGER=1, panel (header and live extent)
    included, and the snapshot unchanged."""
    world = {"inplace": LP.inplace_world, "small": LP.small_world}[which]()
    e = [size for size, _ in world.rings].index(ring)
    assert LP.form(world, e, 3, ring, False) == form
    pair = LZ.Pair(world)
    snaps = pair.start("j")
    active = np.zeros(world.n, dtype=np.uint8)
    active[e] = 1
    stats = pair.run(lambda eng: LZ._restore_step(eng, LZ.JIG, active=torch.tensor(active, device=eng.device)))
    assert stats[0] == stats[1] == (1, 0), stats
    LZ._assert_same(pair, "%s ring %d" % (which, ring), snaps)
    pair.close()
