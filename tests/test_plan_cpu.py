"""The engine's launch planner (occuspytial_amd/csrc/occ_plan.hpp) on the CPU: which form of the fused solve and which CU
partition a shape gets, pinned to what an MI355X chose (profiles/r04_sizes.txt), plus invariants over a grid of shapes.
The planner is built with g++ on demand (`make plan`, occ_plan_capi.cpp) and driven through ctypes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')
NCU = 256
UNSET = -2 ** 31
FORM_STEPS, FORM_ANY, FORM_XCD, FORM_TILES = 0, 1, 2, 3


class Options(C.Structure):  # occ::PlanOptions, field for field
    _fields_ = [(f, C.c_bool) for f in (
        'no_persistent', 'no_tiles', 'no_xcd_local', 'no_scalar_wave', 'no_xcd_shares', 'no_beta_split', 'no_side_stream',
        'stream_events', 'event_sync', 'skip_residency_probe', 'no_dia', 'no_gram32', 'gram32_one_chain', 'break_handover')] + \
        [(f, C.c_int) for f in ('force_tiles', 'tiles_main_cus', 'cold_cus', 'cu_split', 'main_share', 'surplus_last', 'zob_skip',
                                'tiles_gb')]


class Out(C.Structure):  # OccPlanOut of occ_plan_capi.cpp
    _fields_ = [(f, C.c_int32) for f in (
        'form', 'main_cus', 'tpb', 'nb_n', 'nb_r', 'beta_split', 'share_on', 'surplus_last', 'iter_window', 'generic', 'nbg',
        'tiles_T', 'tiles_G', 'xl_wide', 'xl_nbg', 'xl_per_cu', 'main_hot_cus', 'nmain', 'partition', 'flag_sync')] + [
        ('per_xcd', C.c_int32 * 8), ('tile_first', (C.c_int32 * 9) * 3), ('tile_most', C.c_int32 * 3),
        ('n_ladder', C.c_int32), ('ladder_form', C.c_int32 * 4), ('ladder_nbg', C.c_int32 * 4)]


@pytest.fixture(scope='module')
def planner():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    lib = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    lib.occ_plan_eval.restype = C.c_int
    lib.occ_plan_eval.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(Options), C.c_int32, C.POINTER(Out), C.c_char_p, C.c_int32]

    def plan(n, chains, p=2, q=2, rsr_dim=0, wmax=8, dia=True, granted=True, rows=None, ncu=NCU, **knobs):
        """The plan of a shape, settled on its ladder's first form (every form resident, as on an idle device)."""
        opt = Options(force_tiles=UNSET, tiles_main_cus=UNSET, cold_cus=UNSET, cu_split=UNSET, main_share=UNSET, tiles_gb=1)
        for k, v in knobs.items():
            setattr(opt, k, v)
        shape = (C.c_int32 * 8)(n, 2 * n if rows is None else rows, chains, p, q, rsr_dim, wmax, int(dia))
        out, err = Out(), C.create_string_buffer(512)
        if lib.occ_plan_eval(shape, ncu, C.byref(opt), int(granted), C.byref(out), err, 512) != 0:
            raise ValueError(err.value.decode())
        return out
    return plan


# (side, chains, knobs) -> (persistent_solve, main_stream_cus) as the device recorded them (queen lattices, p = q = 2)
PINNED = [
    (20, 1, {}, 2, 160), (60, 8, {}, 2, 160), (60, 24, {}, 2, 160),
    (100, 1, {}, 2, 136), (100, 2, {}, 2, 144), (100, 4, {}, 2, 160), (100, 5, {}, 2, 156),
    (100, 6, {}, 2, 160), (100, 8, {}, 2, 160), (100, 16, {}, 2, 160), (100, 32, {}, 2, 160),
    (150, 2, {}, 1, 176),
    (250, 1, {}, 3, 128), (250, 2, {}, 3, 128), (250, 4, {}, 3, 128), (350, 1, {}, 3, 128), (500, 1, {}, 3, 128),
    (100, 4, {'no_xcd_local': True}, 1, 160),
    (250, 1, {'no_tiles': True}, 1, 160), (250, 2, {'no_tiles': True}, 1, 0), (350, 1, {'no_tiles': True}, 1, 0),
    (500, 1, {'no_tiles': True}, 0, 0),
    (100, 4, {'no_persistent': True}, 0, 0),
]


@pytest.mark.parametrize('side,chains,knobs,form,main_cus', PINNED)
def test_pinned_plans(planner, side, chains, knobs, form, main_cus):
    pl = planner(side * side, chains, **knobs)
    assert (pl.form, pl.main_cus) == (form, main_cus)


def test_scalar_wave_form(planner):
    pl = planner(100 * 100, 4)
    assert (pl.form, pl.xl_wide, pl.main_cus) == (FORM_XCD, 1, 160)
    assert list(pl.per_xcd) == [24] * 4 + [16] * 4
    pl = planner(100 * 100, 4, no_scalar_wave=True)
    assert (pl.form, pl.xl_wide, pl.main_cus) == (FORM_XCD, 2, 160)


def test_wide_rows_take_the_16_window(planner):
    pl = planner(3000, 1, wmax=11, dia=False)
    assert pl.iter_window == 16 and pl.form in (FORM_ANY, FORM_XCD)
    assert planner(3000, 1).iter_window == 8


@pytest.mark.parametrize('p,q', [(12, 2), (2, 12)])
def test_many_covariates_take_the_generic_path(planner, p, q):
    pl = planner(100 * 100, 4, p=p, q=q)
    assert pl.generic and pl.form == FORM_STEPS and pl.main_cus == 0 and pl.n_ladder == 1


def test_reduced_rank_partition(planner):
    for m in (1, 50, 128):
        pl = planner(40 * 50, 4, rsr_dim=m)
        assert (pl.form, pl.main_cus, pl.tpb) == (FORM_STEPS, 192, pl.tpb)
    for m in (129, 1280, 4096):
        pl = planner(100 * 100, 4, rsr_dim=m)
        assert (pl.form, pl.partition, pl.main_cus) == (FORM_STEPS, 0, 0)


@pytest.mark.parametrize('split', [1, 16, 31, 48, 100, 240, 256, -32])
def test_invalid_cu_split(planner, split):
    with pytest.raises(ValueError, match='OCC_CU_SPLIT must be 0 .no partition. or a multiple of 32 that leaves the side stream '
                                         'at least 32 CUs'):
        planner(100 * 100, 4, cu_split=split)


@pytest.mark.parametrize('split,main_cus', [(0, 0), (64, 64), (224, 224)])
def test_valid_cu_split(planner, split, main_cus):
    assert planner(20 * 20, 1, cu_split=split).main_cus == main_cus


GRID_N = [400, 1000, 2500, 6400, 10000, 14000, 22500, 40000, 62500, 122500, 250000]
GRID_C = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32]


@pytest.mark.parametrize('wmax', [8, 16])
@pytest.mark.parametrize('granted', [True, False])
def test_plan_invariants(planner, wmax, granted):
    for n in GRID_N:
        for chains in GRID_C:
            pl = planner(n, chains, wmax=wmax, dia=wmax == 8, granted=granted)
            what = (n, chains, wmax, granted)
            assert pl.tpb in (64, 128, 256), what
            assert pl.ladder_form[pl.n_ladder - 1] == FORM_STEPS, what
            cus = pl.main_cus if pl.main_cus > 0 else NCU
            hot = pl.main_hot_cus if pl.main_cus > 0 else NCU // 8
            for i in range(pl.n_ladder - 1):  # every fused form on the ladder fits arithmetically
                f, nbg = pl.ladder_form[i], pl.ladder_nbg[i]
                if f == FORM_TILES:
                    assert pl.tiles_G * chains <= {1: 4, 2: 3, 3: 3, 4: 2}[pl.tiles_T] * cus, what
                elif f == FORM_XCD:
                    assert pl.xl_nbg <= pl.xl_per_cu * hot, what
                    if pl.main_cus > 0:
                        assert all(c % 4 == 0 for c in pl.per_xcd), (what, list(pl.per_xcd))
                else:
                    assert f == FORM_ANY and nbg * chains <= (2 if pl.iter_window == 8 else 1) * cus, what
            if pl.main_cus > 0:
                assert granted and NCU - pl.main_cus >= 32, what
            if pl.share_on:
                per_chain = [2 * ((n + 255) // 256) if pl.tpb == 64 else 2 * pl.nb_n, pl.nb_r, (n + 255) // 256]
                for k in range(3):
                    first = list(pl.tile_first[k])
                    assert first[0] == 0 and first == sorted(first), what
                    assert first[8] == per_chain[k] * chains, what
