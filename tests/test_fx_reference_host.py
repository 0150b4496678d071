"""Host tests (no GPU) of tests/fx_cases.py: the layouts, ownership rules, effective matrices, references and the real-data bound that tests/test_gpu_fx_paths.py judges
the four streaming storages of the explicit dual operator by are tied to something independent of them -- each other, the definitions, and the library's host-only entries."""
import ctypes as C

import numpy as np
import pytest

import fx_cases as fc

SMALL = [n for n, c in fc.CASES.items() if max(u if isinstance(u, int) else u[0] for u in c.units) <= 1400]
SIZES = {"full": (1, 33, 129, 260), "sym": (1, 33, 127, 128, 129, 300, 700), "class": (1, 100, 129, 300), "class_sym": (1, 100, 257, 600)}


@pytest.mark.parametrize("storage", fc.STORAGES)
def test_pack_unpack_and_pads(storage):
    """Pack followed by unpack is the effective matrix (the identity on what the storage keeps); every offset is hit at most once and stays inside the allocation; the
    pads are exactly the offsets no (row, column) maps to and they hold zero; the sizes are fx_band_off(npad / 32) resp. 256^2 nsb (nsb + 1) / 2."""
    rng = np.random.default_rng(1)
    for n in SIZES[storage]:
        W = rng.integers(1, 9, size=(n, n)).astype(np.float64)
        p, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        keep = fc.stored_mask(storage, n, p, c)
        off = fc.offsets(storage, n, p[keep], c[keep])
        size = fc.storage_size(storage, n)
        assert np.unique(off).size == off.size and off.min() >= 0 and off.max() < size
        img = fc.pack(storage, W)
        pads = np.ones(size, dtype=bool)
        pads[off] = False
        assert not np.any(img[pads]) and np.all(img[~pads] != 0)
        back = fc.unpack(storage, n, img)
        assert np.array_equal(back, W if storage == "class" else fc.effective(storage, W))
        ld = fc.ld_of(storage, n)
        if storage == "sym":
            assert size == fc.fx_band_off(ld // 32) == 4096 * sum(k // 4 + 1 for k in range(ld // 32))  # band k: k // 4 + 1 tiles of 32 x 128
        elif storage == "class_sym":
            nsb = ld // 256
            assert size == 256 * 256 * nsb * (nsb + 1) // 2
        else:
            assert size == ld * ld


@pytest.mark.parametrize("storage", fc.STORAGES)
def test_effective_matrices(storage):
    """E equals W for symmetric W; for an unsymmetric W it is what the rule says entry by entry (restated here with plain loops)."""
    rng = np.random.default_rng(2)
    for n in (5, 70, 131):
        A = rng.integers(1, 9, size=(n, n))
        S = np.tril(A) + np.tril(A, -1).T
        assert np.array_equal(fc.effective(storage, S), S)
        E = fc.effective(storage, A)
        for p in range(n):
            for c in range(n):
                if storage == "full":
                    want = A[p, c]
                elif storage == "class":
                    want = A[c, p]
                elif storage == "sym":
                    hi, lo = (p, c) if p // 32 >= c // 32 else (c, p)
                    want = A[p, c] if p // 32 == c // 32 else A[hi, lo]
                else:
                    want = A[max(p, c), min(p, c)]
                assert E[p, c] == want


@pytest.mark.parametrize("name", SMALL)
def test_references(name):
    """The range-by-range reference equals the dense effective-matrix product block by block; the integer reference equals the long-double one; a float64 numpy product
    stays inside the real-data bound (the reference alone does); the image built by ranges equals the packed whole."""
    d = fc.data(name)
    xs = d.X()
    ref, _ = d.reference(xs)
    refl, _ = d.reference(xs, dtype=np.longdouble)
    assert np.array_equal(ref.astype(np.longdouble), refl)
    for b in range(d.nblocks):
        u = d.unit_of(b)
        E = fc.effective(d.storage, d.W(u))[np.ix_(d.pos[b], d.pos[b])]
        assert np.array_equal(ref[d.index(b)], E @ xs[b])
    assert not np.any(ref[~d.column_mask()])
    xr = d.X(real=True)
    rr, mag = d.reference(xr, real=True)
    y = np.zeros(d.nX)
    for b in range(d.nblocks):
        E = fc.effective(d.storage, d.W(d.unit_of(b), real=True))
        y[d.column(b)] = (E[:, d.pos[b]] if d.cls else E[np.ix_(d.pos[b], d.pos[b])]) @ xr[b]  # (class storages: the whole column of W_c X)
    assert np.all(np.abs(y.astype(np.longdouble) - rr) <= d.bound(mag))
    for u, n in enumerate(d.n_unit):
        if n:
            assert np.array_equal(d.image(u), fc.pack(d.storage, d.W(u).astype(np.float64)))


@pytest.mark.parametrize("name,size", [("sym_129_300", 2), ("sym_129_300", 3), ("sym_100_100", 8), ("class_300", 3), ("class_100", 8), ("csym_2_megabands", 8), ("csym_1300", 2)])
def test_shares_sum_to_the_whole(name, size):
    """The stripe ranks' references and images add up to the whole ones, every row has exactly one owner."""
    d = fc.data(name)
    xs = d.X()
    whole, _ = d.reference(xs)
    assert np.array_equal(sum(d.reference(xs, stripe=(r, size))[0] for r in range(size)), whole)
    for u, n in enumerate(d.n_unit):
        if n:
            assert np.array_equal(sum(fc.owned_rows(d.storage, d.n_unit, u, (r, size)).astype(int) for r in range(size)), np.ones(n, dtype=int))
            assert np.array_equal(sum(d.image(u, stripe=(r, size)) for r in range(size)), d.image(u))


def test_ownership_rules_equal_the_library():
    """fx_stripe_plan and the mega-band snake order as restated here against pmh_fexplicit_stripe_owner / pmh_fexplicit_class_sym_plan (host only, no device); the row
    ranges of "class" cover the padded rows once, in groups of 32."""
    import permon_amd as pa

    L = pa.load()
    for ngam in ([129, 300], [100, 100], [4230], [5, 0, 260], [700, 33, 1, 900]):
        for size in (1, 2, 3, 8):
            ng = np.array(ngam, dtype=np.int32)
            out = np.full(sum(-(-n // 128) for n in ngam), -1, dtype=np.int32)
            pa._lib.check(L.pmh_fexplicit_stripe_owner(len(ngam), ng.ctypes.data_as(C.c_void_p), size, out.ctypes.data_as(C.c_void_p)))
            assert np.array_equal(out, np.concatenate(fc.sym_stripe_owner(ngam, size)))
    for n_c in (100, 1025, 1100, 3100, 8200, 33288):
        for size in (1, 2, 3, 8):
            mine = fc.class_sym_owner(n_c, size)
            out = np.full(mine.size, -1, dtype=np.int32)
            pa._lib.check(L.pmh_fexplicit_class_sym_plan(n_c, size, out.ctypes.data_as(C.c_void_p), None))
            assert np.array_equal(out, mine)
    for n_c in (100, 300, 700):
        for size in (1, 3, 8):
            r = [fc.class_row_range(n_c, k, size) for k in range(size)]
            assert r[0][0] == 0 and r[-1][1] == fc.pad_to(n_c, 128) and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(a % 32 == 0 and b % 32 == 0 for a, b in r)


def test_group_case_is_invariant():
    """The order-4 group of csym_group: four distinct signed permutations closed under composition, and W invariant under each (integer and real)."""
    d = fc.data("csym_group")
    pm, sg = d.sym_group[0]
    n = d.n_unit[0]
    assert np.array_equal(pm[0], np.arange(n)) and np.all(sg[0] == 1) and len({tuple(q) for q in pm}) == 4
    for g in range(4):
        for h in range(4):
            comp_p, comp_s = pm[g][pm[h]], sg[h] * sg[g][pm[h]]
            assert any(np.array_equal(comp_p, pm[k]) and np.array_equal(comp_s, sg[k]) for k in range(4))
    for real in (False, True):
        W = d.W(0, real)
        assert np.array_equal(W, W.T) and np.mean(W != 0) > 0.5 and (real or np.abs(W).max() <= 8)
        for g in range(4):
            assert np.array_equal(W[np.ix_(pm[g], pm[g])], sg[g][:, None] * sg[g][None, :] * W)
