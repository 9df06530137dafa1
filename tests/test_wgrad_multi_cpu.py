"""CPU test of the multi-job weight-gradient launch plan (csrc/gemm_km.hip, no GPU): wc_gemm_km_multi_plan gives the launches,
wc_gemm_km_multi_locate runs the KERNEL's own table, job search and (unit, tile) arithmetic on the host for one workgroup id.
Over random job lists every (job, unit, tile) must be computed by exactly one workgroup, every job must start at a multiple of
8 (the XCD a workgroup lands on is its id mod 8), jobs run longest K loop first and chunking keeps that order."""
import ctypes
import random

import pytest

from weclip_vit_comer_amd import _lib, ops

CUS = 256
KMJ_MAX = 32          # jobs per launch (csrc/gemm_km.hip)


def _job(rng, k):
    M = rng.choice([64, 70, 600, 1000, 1024, 2048, 4096])
    N = rng.choice([21, 64, 130, 256, 300])
    K = rng.choice([64, 128, 200, 256, 320, 512])
    mslice = 64 * rng.choice([1, 2, 4, 8, 16, 100])
    if M // mslice > 16:
        mslice = (M // 16 + 63) // 64 * 64
    groups = rng.choice([1, 1, 1, 2, 3, 8])
    lda = (N * groups + 7) // 8 * 8 + rng.choice([0, 8])
    ldx = (K + 7) // 8 * 8
    base = 0x10000 * (3 * k + 1)
    return [base, base + 0x10000, base + 0x20000, M, N, K, lda, ldx, max(M, 64), 0, 0, mslice, rng.choice([0, 1]), groups,
            (N + 7) // 8 * 8 if groups > 1 else 0, 0]


def _plan(jobs):
    n = len(jobs)
    flat = (ctypes.c_int64 * (16 * n))(*[v for j in jobs for v in j])
    launch, first, pos = ((ctypes.c_int * n)() for _ in range(3))
    cap = 2 * (n // KMJ_MAX + 1)
    grids, forms = (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    nl = ctypes.c_int(0)
    _lib.lib().wc_gemm_km_multi_plan(flat, n, CUS, launch, first, pos, grids, forms, cap, ctypes.byref(nl))
    return flat, list(launch), list(first), list(pos), list(grids)[:nl.value], list(forms)[:nl.value]


def _shape(j):
    M, N, K, mslice, bias, groups = j[3], j[4], j[5], j[11], j[12], j[13]
    ns = -(-M // mslice)
    tiles = ops.wgrad_tiles(N, K, bias=bool(bias))
    return ns, tiles, groups * ns


@pytest.mark.parametrize("seed,count", [(0, 5), (1, 33), (2, 70)])
def test_every_unit_and_tile_has_exactly_one_workgroup(seed, count):
    rng = random.Random(seed)
    jobs = [_job(rng, k) for k in range(count)]
    flat, launch, first, pos, grids, forms = _plan(jobs)
    assert len(grids) >= -(-count // KMJ_MAX)
    lib = _lib.lib()
    out = (ctypes.c_int * 3)()
    owners = {}
    for l, grid in enumerate(grids):
        assert grid % 8 == 0
        for wg in range(grid):
            lib.wc_gemm_km_multi_locate(flat, count, CUS, l, wg, out)
            q, unit, tile = out[0], out[1], out[2]
            if q < 0:
                continue
            assert launch[q] == l and first[q] <= wg
            ns, tiles, units = _shape(jobs[q])
            assert 0 <= unit < units and 0 <= tile < tiles
            if units % 8 == 0:      # XCD-aware order: all tiles of a unit on the XCD (id mod 8) of its number
                assert unit % 8 == wg % 8
            key = (q, unit, tile)
            assert key not in owners, (key, owners[key], (l, wg))
            owners[key] = (l, wg)
    for q, j in enumerate(jobs):
        ns, tiles, units = _shape(j)
        assert first[q] % 8 == 0
        assert all((q, u, t) in owners for u in range(units) for t in range(tiles)), q
    assert len(owners) == sum(_shape(j)[1] * _shape(j)[2] for j in jobs)


@pytest.mark.parametrize("seed,count", [(3, 40), (4, 100)])
def test_order_forms_and_chunks(seed, count):
    rng = random.Random(seed)
    jobs = [_job(rng, k) for k in range(count)]
    _, launch, first, pos, grids, forms = _plan(jobs)
    length = lambda j: min(j[3], j[11])           # tokens of one workgroup's K loop
    form = lambda j: 2 if (_shape(j)[1] * _shape(j)[2] <= CUS and j[11] >= 128) else 1
    for f in (1, 2):
        mine = [q for q in range(count) if form(jobs[q]) == f]
        ls = [l for l in range(len(grids)) if forms[l] == f]
        assert sorted({launch[q] for q in mine}) == ls and len(ls) == -(-len(mine) // KMJ_MAX)
        ran = sorted(mine, key=lambda q: (launch[q], pos[q]))
        assert ran == sorted(mine, key=lambda q: -length(jobs[q]))        # longest first; stable: equal lengths keep the input order
        for l in ls:
            here = [q for q in ran if launch[q] == l]
            assert [pos[q] for q in here] == list(range(len(here))) and len(here) <= KMJ_MAX
            nxt = 0
            for q in here:                         # back to back, each start rounded up to a multiple of 8
                assert first[q] == nxt
                nxt += (_shape(jobs[q])[1] * _shape(jobs[q])[2] + 7) // 8 * 8
            assert grids[l] == nxt


def test_bad_jobs_are_reported():
    rng = random.Random(9)
    j = _job(rng, 0)
    for field, value, msg in [(11, 100, "mslice"), (6, j[4] - 1 if j[4] % 8 else j[4] - 8, "16-byte aligned"), (0, 0, "bad argument")]:
        bad = list(j)
        bad[field] = value
        with pytest.raises(RuntimeError, match=msg):
            _plan([bad])
