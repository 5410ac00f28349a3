"""Plan and execution agree on where the result lands (run with -m gpu on an MI355X): relax on a level, then both of
the level's arrays must hold what the plan of ndsm_hip_debug_relax_plan says - the array named as the result the
swept field, its partner the state an out-of-place pass last read from it (or what it held before the call where no
pass ever wrote it).  Bit for bit against the in-place colour passes; the parity tests pin the values themselves."""
import numpy as np
import pytest

import plan_tools
from golden_inputs import rand_field, uniform_mesh

pytestmark = pytest.mark.gpu

BCS = "NDDNDD"
# Fortran order: a block level, a thin level that only the forced fused launch takes, the smallest block level
CASES = (([64, 64, 64], "OP_RELAX", 0), ([128, 16, 16], "OP_RELAX_FUSED", 2), ([17, 16, 16], "OP_RELAX", 0))
COUNTS = (1, 2, 5)


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


@pytest.mark.parametrize("ns,op,variant", CASES, ids=["x".join(map(str, c[0])) for c in CASES])
def test_result_buffer_is_the_planned_one(hip, ns, op, variant):
    shp = tuple(ns[::-1])
    u, rhs, mark = rand_field(shp, 4101), rand_field(shp, 4102), rand_field(shp, 4103)
    S = hip.MGSolver(ns, uniform_mesh(ns), BCS)
    S.upload(1, hip.BUF_RHS, rhs)
    S.upload(1, hip.BUF_U, u)
    state = [u]                                   # after k sweeps, by the in-place colour passes
    for _ in range(max(COUNTS)):
        S.op(hip.OP_RELAX_COLOR, 1, 1)
        state.append(S.download(1, hip.BUF_U))
    lb = [int(BCS[d] == "D") for d in range(3)]
    ub = [ns[d] - 1 - int(BCS[3 + d] == "D") for d in range(3)]
    for n in COUNTS:
        plan = plan_tools.relax_plan(ns, n, lb=lb, ub=ub, variant=variant)
        assert plan["err"] == 0 and sum(q["sweeps"] for q in plan["passes"]) == n
        holds = {0: 0, 1: None}                   # sweeps behind the content of either array; None: the mark
        for q in plan["passes"]:
            holds[q["dst"]] = holds[q["src"]] + q["sweeps"]
        assert holds[plan["result"]] == n
        assert plan["result"] == 1, "these cases are meant to end in the partner array"
        S.upload(1, hip.BUF_U, u)                 # array 0 of this call, whichever it was before
        S.upload(1, hip.BUF_UALT, mark)
        S.op(getattr(hip, op), 1, n)
        assert np.array_equal(S.download(1, hip.BUF_U), state[n]), (ns, n)
        other = holds[1 - plan["result"]]
        assert np.array_equal(S.download(1, hip.BUF_UALT), mark if other is None else state[other]), (ns, n, other)
    # an in-place plan leaves the partner alone
    plan = plan_tools.relax_plan(ns, 2, lb=lb, ub=ub, variant=1)
    assert plan["result"] == 0 and [q["kind"] for q in plan["passes"]] == ["color3d"] * 2
    S.upload(1, hip.BUF_U, u)
    S.upload(1, hip.BUF_UALT, mark)
    S.op(hip.OP_RELAX_COLOR, 1, 2)
    assert np.array_equal(S.download(1, hip.BUF_U), state[2])
    assert np.array_equal(S.download(1, hip.BUF_UALT), mark)
    S.close()
