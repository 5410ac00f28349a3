"""CPU tests of the numpy restatements of the flux partitioning and connectivity semantics (tests/connect_model.py) on
closed forms: what the restatements say is what include/ndsm_hip.h means, before the device is held to their bits
(test_gpu_connect.py)."""
import numpy as np
import pytest

import connect_model as cm
import line_model

EPS = np.finfo(np.float64).eps


def gaussians(nx=33, ny=25):
    """two equal positive Gaussians, mirror images about the pixel column x = 0, and a negative one below them"""
    xs, ys = np.linspace(-4.0, 4.0, nx), np.linspace(-3.0, 3.0, ny)
    X, Y = np.meshgrid(xs, ys)
    g = lambda x0, y0: np.exp(-((X - x0) ** 2 + (Y - y0) ** 2))
    return xs, ys, g(-1.5, 0.75) + g(1.5, 0.75) - g(0.0, -1.5)


def arcade_plane(nx=31, ny=9):
    xs, ys = np.linspace(-1.5, 1.5, nx), np.linspace(0.0, 1.0, ny)
    return xs, ys, np.broadcast_to(-np.sin(xs)[None, :], (ny, nx)).copy()     # (one row's values: the ties are exact)


def ramp(nx, ny):
    xs, ys = np.arange(float(nx)), np.arange(float(ny))
    return xs, ys, np.broadcast_to(1.0 + np.arange(float(nx))[None, :], (ny, nx)).copy()


def snake(nx=18, ny=7):
    """one patch whose pointer chain winds through every other row: longer than half the magnetogram"""
    xs, ys = np.arange(float(nx)), np.arange(float(ny))
    bz = np.zeros((ny, nx))
    v = 1.0
    for j in range(0, ny, 2):
        cols = range(nx) if (j // 2) % 2 == 0 else range(nx - 1, -1, -1)
        for i in cols:
            bz[j, i] = v
            v += 1.0
        if j + 1 < ny:
            bz[j + 1, nx - 1 if (j // 2) % 2 == 0 else 0] = v
            v += 1.0
    return xs, ys, bz


def noise(nx, ny, seed=1):
    rng = np.random.default_rng(seed)
    return np.arange(float(nx)), 0.5 * np.arange(float(ny)), rng.uniform(-1.0, 1.0, (ny, nx))


def arcade_field(nx, ny, nz, zmax=1.5):
    x, y, z = np.linspace(-1.5, 1.5, nx), np.linspace(0.0, 1.0, ny), np.linspace(0.0, zmax, nz)
    X, _Y, Z = line_model.grids((x, y, z))
    b = np.stack([np.cos(X) * np.exp(-Z), np.zeros_like(X), -np.sin(X) * np.exp(-Z)])
    return (x, y, z), b


def test_three_gaussians_three_patches_and_the_tie_rule():
    xs, ys, bz = gaussians()
    P = cm.partition_numpy(xs, ys, bz, 0.05)
    assert P["K"] == 3
    peaks = sorted(int(np.argmax(np.where(m, np.abs(bz), 0.0))) for m in
                   ((bz > 0) & (xs[None, :] < 0), (bz > 0) & (xs[None, :] > 0), bz < 0))
    assert list(P["root"]) == peaks
    assert list(P["sign"]) == [-1, 1, 1]              # the negative peak lies in the lowest rows
    mid = list(xs).index(0.0)
    col = P["label"][:, mid]
    left = P["label"][np.nonzero(col)[0], mid - 1]
    assert (col[bz[:, mid] > 0.05] == 2).all() and 3 not in col      # the boundary column goes to the lower root index
    assert set(left[bz[np.nonzero(col)[0], mid] > 0]) == {2}
    assert P["nin"] == int((np.abs(bz) > 0.05).sum()) == int(P["npix"].sum())


def test_arcade_two_patches_rooted_at_the_corners():
    xs, ys, bz = arcade_plane()
    P = cm.partition_numpy(xs, ys, bz, 0.0)
    assert P["K"] == 2 and list(P["root"]) == [0, 30] and list(P["sign"]) == [1, -1]
    assert (P["label"][:, 15] == 0).all() and P["nin"] == 30 * 9


@pytest.mark.parametrize("make, chain", [(lambda: ramp(300, 3), 299), (lambda: ramp(1100, 2), 1099), (snake, 68)])
def test_long_pointer_chains_reach_one_root(make, chain):
    xs, ys, bz = make()
    P = cm.partition_numpy(xs, ys, bz, 0.0)
    assert P["K"] == 1 and P["root"][0] == int(np.argmax(bz))
    p, hops = int(np.argmin(np.where(bz > 0, bz, np.inf))), 0
    while P["ptr"][p] != p:
        p, hops = int(P["ptr"][p]), hops + 1
    assert hops == chain
    if make is snake:                                 # more hops than one jumping round too few can cover
        assert hops > 2 ** (int(bz.size).bit_length() - 1)


def test_noise_pointers_ascend_and_labels_follow_them():
    xs, ys, bz = noise(70, 63)
    P = cm.partition_numpy(xs, ys, bz, 0.0)
    assert P["K"] == K_NOISE_70x63
    a, lab = np.abs(bz).reshape(-1), P["label"].reshape(-1)
    inn = np.nonzero(P["ptr"] >= 0)[0]
    assert (a[P["root_of"][inn]] >= a[inn]).all()
    assert (lab[P["ptr"][inn]] == lab[inn]).all() and (lab[inn] > 0).all()
    assert ((bz.reshape(-1)[P["ptr"][inn]] > 0) == (bz.reshape(-1)[inn] > 0)).all()


K_NOISE_70x63 = 985                               # (default_rng(1).uniform(-1, 1, (63, 70)); pinned for this seed)


def test_partition_against_a_pixel_by_pixel_loop():
    """the nine shifted comparisons against the definition read out pixel by pixel, with exact ties in the data"""
    xs, ys, bz = noise(20, 17, seed=3)
    bz = np.round(bz * 4.0) / 4.0                   # nine levels: plateaus and ties everywhere
    bz[3, 4], bz[9, 9] = np.nan, np.inf
    ny, nx = bz.shape
    thr = 0.25
    ptr = np.full(nx * ny, -1)
    for j in range(ny):
        for i in range(nx):
            v = bz[j, i]
            if not abs(v) > thr:
                continue
            cand = [(jj * nx + ii) for jj in (j - 1, j, j + 1) for ii in (i - 1, i, i + 1)
                    if 0 <= ii < nx and 0 <= jj < ny and abs(bz[jj, ii]) > thr and (bz[jj, ii] > 0) == (v > 0)]
            ptr[j * nx + i] = max(cand, key=lambda q: (abs(bz.reshape(-1)[q]), -q))
    P = cm.partition_numpy(xs, ys, bz, thr)
    assert np.array_equal(P["ptr"], ptr)
    root = ptr.copy()
    for p in range(nx * ny):
        while root[p] >= 0 and ptr[root[p]] != root[p]:
            root[p] = ptr[root[p]]
    assert np.array_equal(P["root_of"], root)
    roots = sorted(set(root[root >= 0].tolist()))
    assert list(P["root"]) == roots and P["label"][9, 9] == roots.index(9 * nx + 9) + 1 and P["label"][3, 4] == 0
    assert np.array_equal(P["label"].reshape(-1), [0 if r < 0 else roots.index(r) + 1 for r in root])


def test_keysum_is_the_lane_and_tree_order():
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 6, 1000)
    t = rng.uniform(-1, 1, 1000) * 10.0 ** rng.integers(-8, 8, 1000)
    got = cm.keysum_numpy(keys, t, 5)
    for k in range(1, 6):
        r = t[keys == k]
        v = [0.0] * 64
        for q, val in enumerate(r):                   # ascending rank: lane q % 64 takes it after q - 64
            v[q % 64] = v[q % 64] + val
        d = 32
        while d:
            for l in range(d):
                v[l] = v[l] + v[l + d]
            d //= 2
        assert got[k - 1] == v[0]
    assert np.signbit(cm.keysum_numpy([1, 2], [-0.0, 3.0], 2)[0]) == False and cm.keysum_numpy([1], [7.5], 1)[0] == 7.5


def test_patch_fluxes_add_up_to_the_plane():
    xs, ys, bz = noise(70, 63)
    P = cm.partition_numpy(xs, ys, bz, 0.2)
    f = bz.reshape(-1) * cm.trap_weights(xs, ys)
    inn = np.abs(bz.reshape(-1)) > 0.2
    assert abs(P["flux"].sum() - f[inn].sum()) <= 16 * EPS * np.abs(f[inn]).sum()


@pytest.fixture(scope="module")
def arcade():
    out = {}
    for nx, nz in ((31, 16), (61, 31)):
        mesh, b = arcade_field(nx, 5, nz)
        P = cm.partition_numpy(mesh[0], mesh[1], b[2, 0], 0.0)
        out[nx] = (mesh, b, P, cm.connect_numpy(mesh, b, P["label"], P["K"], 0.5, 4000))
    return out


# the relative gap |Psi(1->2) - Psi(2->1)| / Psi(1->2) of the restatement was measured at 31 x 5 x 16 and 61 x 5 x 31
# as 2.846e-16 and 2.935e-16 (DESIGN.md "Flux partitioning and connectivity" holds both figures): the field is its own
# mirror image, so the closed lines land on mirrored pixels and only the order of the sums differs.  The bounds are ten
# times the measured values.
ARCADE_GAP = {31: 10 * 2.846e-16, 61: 10 * 2.935e-16}


def test_arcade_connectivity_pairs_and_their_balance(arcade):
    for nx, (mesh, b, P, C) in arcade.items():
        assert P["K"] == 2
        pairs = list(zip(C["pa"].tolist(), C["pc"].tolist()))
        assert (1, 2) in pairs and (2, 1) in pairs
        assert all(c < 0 or (a, c) in ((1, 2), (2, 1)) for a, c in pairs), pairs
        assert pairs == sorted(pairs)
        psi = dict(zip(pairs, C["pflux"]))
        gap = abs(psi[(1, 2)] - psi[(2, 1)]) / psi[(1, 2)]
        print("arcade nx = %d: Psi(1->2) = %.17g, Psi(2->1) = %.17g, relative gap %.3e" % (nx, psi[(1, 2)], psi[(2, 1)], gap))
        assert gap <= ARCADE_GAP[nx]
        # every foot's flux is in exactly one pair of its patch
        term = np.abs(b[2, 0].reshape(-1)) * cm.trap_weights(mesh[0], mesh[1])
        lab = P["label"].reshape(-1)
        for a in (1, 2):
            feet = term[(lab == a) & (C["dest"] != cm.CONNECT_NONE)]
            total = sum(f for (pa, _c), f in psi.items() if pa == a)
            assert abs(total - feet.sum()) <= 16 * EPS * feet.sum()
        assert C["ntraced"] == int(C["nlines"].sum()) == int((C["dest"] != cm.CONNECT_NONE).sum())


def test_connect_dest_follows_the_status(arcade):
    mesh, b, P, C = arcade[31]
    st, dest = C["status"], C["dest"]
    traced = dest != cm.CONNECT_NONE
    assert (dest[traced & (st != cm.ZLO)] == -st[traced & (st != cm.ZLO)]).all()
    assert (st[~traced] == line_model.OUTSIDE).all() and (C["length"][~traced] == 0).all()
    assert set(dest[traced & (st == cm.ZLO)]) <= {0, 1, 2}
    # labels outside 1 .. K count as 0: with K = 1 patch 2 is unlabelled ground
    C1 = cm.connect_numpy(mesh, b, P["label"], 1, 0.5, 4000)
    assert set(C1["pa"].tolist()) == {1} and (C1["dest"][P["label"].reshape(-1) == 2] == cm.CONNECT_NONE).all()
    assert 0 in C1["pc"].tolist()
