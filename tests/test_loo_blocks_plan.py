"""sampler.block_plan: the three spellings of Sampler.loo_blocks's blocks turned into the flat lists of bfmmm_chain_loo_blocks, and
the refusals of the Python layer.  No device."""
import numpy as np
import pytest

from bayesfmmm_amd.sampler import BLOCK_MAX, block_plan

NI = [5, 1, 23, 64, 130]


def _blocks(plan):
    bc, bo, bx = plan
    assert bc.dtype == np.int32 and bo.dtype == np.int64 and bx.dtype == np.int32
    assert bo[0] == 0 and len(bo) == len(bc) + 1 and bo[-1] == len(bx)
    return [(int(bc[k]), [int(v) for v in bx[bo[k]:bo[k + 1]]]) for k in range(len(bc))]


def test_explicit_blocks_keep_their_order():
    spelled = [(0, [3, 4, 2]), (4, range(10, 30)), (0, [0]), (2, np.arange(22, 0, -3))]
    got = _blocks(block_plan(NI, blocks=spelled))
    assert got == [(0, [3, 4, 2]), (4, list(range(10, 30))), (0, [0]), (2, list(range(22, 0, -3)))]


def test_block_size_cuts_every_curve_with_a_last_short_block():
    got = _blocks(block_plan(NI, block_size=10))
    want = []
    for i, m in enumerate(NI):
        want += [(i, list(range(j, min(j + 10, m)))) for j in range(0, m, 10)]
    assert got == want
    assert [len(b) for i, b in got if i == 2] == [10, 10, 3] and [len(b) for i, b in got if i == 1] == [1]
    assert _blocks(block_plan(NI, block_size=BLOCK_MAX))[-3:] == [(4, list(range(0, 64))), (4, list(range(64, 128))), (4, [128, 129])]
    assert all(len(b) == 1 for _, b in _blocks(block_plan(NI, block_size=1)))


def test_curves_order_and_repeats():
    got = _blocks(block_plan(NI, block_size=4, curves=[2, 0, 2]))
    two = [(2, list(range(j, min(j + 4, 23)))) for j in range(0, 23, 4)]
    assert got == two + [(0, [0, 1, 2, 3]), (0, [4])] + two
    assert _blocks(block_plan(NI, horizon=3, curves=[4, 0, 4])) == [(4, [127, 128, 129]), (0, [2, 3, 4]), (4, [127, 128, 129])]


def test_horizon():
    assert _blocks(block_plan(NI, horizon=4, curves=[0, 2, 3])) == [(0, [1, 2, 3, 4]), (2, [19, 20, 21, 22]), (3, [60, 61, 62, 63])]
    with pytest.raises(ValueError, match="curve 1 has 1 observations"):
        block_plan(NI, horizon=1)
    with pytest.raises(ValueError, match="curve 0 has 5 observations"):       # n_i > h is needed: the rest must not be empty
        block_plan(NI, horizon=5, curves=[2, 0, 1])
    with pytest.raises(ValueError, match="'horizon'"):
        block_plan(NI, horizon=0, curves=[2])
    with pytest.raises(ValueError, match="'horizon'"):
        block_plan(NI, horizon=65, curves=[4])


def test_refusals():
    with pytest.raises(ValueError, match="exactly one"):
        block_plan(NI)
    with pytest.raises(ValueError, match="exactly one"):
        block_plan(NI, blocks=[(0, [1])], block_size=2)
    with pytest.raises(ValueError, match="exactly one"):
        block_plan(NI, block_size=2, horizon=2)
    with pytest.raises(ValueError, match="'curves' goes with"):
        block_plan(NI, blocks=[(0, [1])], curves=[0])
    with pytest.raises(ValueError, match="block 1 has 0 observations"):
        block_plan(NI, blocks=[(0, [1]), (2, [])])
    with pytest.raises(ValueError, match="block 0 has 65 observations"):
        block_plan(NI, blocks=[(4, range(65))])
    assert _blocks(block_plan(NI, blocks=[(4, range(64))])) == [(4, list(range(64)))]
    with pytest.raises(ValueError, match="'block_size'"):
        block_plan(NI, block_size=0)
    with pytest.raises(ValueError, match="'block_size'"):
        block_plan(NI, block_size=65)
    with pytest.raises(ValueError, match="block 0 repeats an index"):
        block_plan(NI, blocks=[(2, [3, 7, 3])])
    with pytest.raises(ValueError, match="block 0: an index outside 0 .. 4 of curve 0"):
        block_plan(NI, blocks=[(0, [5])])
    with pytest.raises(ValueError, match="an index outside"):
        block_plan(NI, blocks=[(0, [-1])])
    with pytest.raises(ValueError, match="block 1: curve 5 outside 0 .. 4"):
        block_plan(NI, blocks=[(0, [0]), (5, [0])])
    with pytest.raises(ValueError, match="'curves' must lie"):
        block_plan(NI, block_size=3, curves=[0, 5])
    with pytest.raises(ValueError, match="no blocks"):
        block_plan(NI, blocks=[])
