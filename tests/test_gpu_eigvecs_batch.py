"""Eigenvector blocks of a whole batch of channels in one call (bspatom_eigvecs_batch / _dev, csrc/eigvec.hip::invit_batch_kernel):
bit for bit the per-channel bspatom_eigvecs, its argument checks, the C4 scale, the all-vectors rate against the per-channel loop,
and Eigenvec_All.dat unchanged through both hosts."""
import os
import subprocess
import time
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from conftest import ROOT, golden_input
from test_gpu_stages import input_from_case, note

from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu


def _odd_block(nfun, cap=37):
    count = min(cap, nfun - 1)
    return count if count % 2 else count - 1


def band_mv(B, X):
    """M X for the symmetric band B[d, i] = M(i, i + d) (d = 0 .. k-1, the layout of bspatom_assemble); X: (n, m)"""
    k, n = B.shape
    Y = B[0][:, None] * X
    for d in range(1, k):
        Y[:n - d] += B[d, :n - d, None] * X[d:]
        Y[d:] += B[d, :n - d, None] * X[:n - d]
    return Y


@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "bsp0", "c1_lin", "lin256", "bc10", "c5_1024_k11"])
def test_eigvecs_batch_bit_identical_to_per_channel(name):
    """Channels 1 .. lmax, vectors 2 .. count + 1 (count odd): np.array_equal with eigvecs per channel.  c5_1024_k11 has
    k = 11 (the BT = 15 instance of the kernel), the others k <= 9 (BT = 8)."""
    prob = capi.Problem(input_from_case(name))
    nch = prob.lmax + 1
    assert nch >= 2
    E, info = prob.solve(0, nch)
    assert np.all(info == 0)
    l0, nl, n0, count = 1, nch - 1, 2, _odd_block(prob.nfun)
    Z = prob.eigvecs_batch(l0, nl, n0, count)
    assert Z.shape == (nl, count, prob.nfun)
    R = np.stack([prob.eigvecs(l, n0, count) for l in range(l0, l0 + nl)])
    assert np.array_equal(Z, R), (name, np.max(np.abs(Z - R)))
    # and the whole range from channel 0, vector 1
    assert np.array_equal(prob.eigvecs_batch(0, nch, 1, 3), np.stack([prob.eigvecs(l, 1, 3) for l in range(nch)]))
    prob.close()


def test_eigvecs_batch_dev_equals_host_variant():
    prob = capi.Problem(input_from_case("lin256"))
    nch = prob.lmax + 1
    prob.solve(0, nch)
    l0, nl, n0, count = 1, nch - 1, 3, 101
    Zh = prob.eigvecs_batch(l0, nl, n0, count)
    Zd = torch.full((nl, count, prob.nfun), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    prob.eigvecs_batch_dev(l0, nl, n0, count, Zd.data_ptr())
    assert np.array_equal(Zd.cpu().numpy(), Zh)
    prob.close()


def test_eigvecs_batch_argument_checks():
    prob = capi.Problem(input_from_case("c1_lin"))
    nch, n = prob.lmax + 1, prob.nfun
    prob.solve(0, nch)
    Zd = torch.zeros((2, 2, n), dtype=torch.float64, device="cuda:0")
    bad = [(nch - 1, 2, 1, 1),          # channel nch outside the last solve
           (-1, 1, 1, 1),               # channel -1
           (0, 0, 1, 1),                # nl = 0
           (0, 1, 1, 0),                # count = 0
           (0, 1, 0, 1),                # n0 = 0
           (0, 1, n, 2)]                # n0 + count - 1 > nfun
    for a in bad:
        with pytest.raises(capi.BspAtomError) as ei:
            prob.eigvecs_batch(*a)
        assert ei.value.code == -2, a
        with pytest.raises(capi.BspAtomError) as ei:
            prob.eigvecs_batch_dev(*a, Zd.data_ptr())
        assert ei.value.code == -2, a
    prob.eigvecs_batch(0, nch, 1, 2)                             # valid
    prob.assemble(0, nch)                                        # invalidates the state of the last solve
    for call in (lambda: prob.eigvecs_batch(0, 1, 1, 1), lambda: prob.eigvecs_batch_dev(0, 1, 1, 1, Zd.data_ptr())):
        with pytest.raises(capi.BspAtomError) as ei:
            call()
        assert ei.value.code == -2
    prob.close()


@pytest.fixture(scope="module")
def c4():
    """C4: n = 4096, k = 9, 128 channels, assembled (the bands for the checks) and then solved"""
    prob = capi.Problem(input_from_case("c4_4096", l_fin=127))
    assert prob.nfun == 4096 and prob.lmax == 127
    SB, HB = prob.assemble(0, 128)
    E, info = prob.solve(0, 128)
    assert np.all(info == 0)
    yield prob, SB, HB, E
    prob.close()


def test_eigvecs_batch_c4_scale(c4):
    """128 channels x 64 vectors at n = 4096 in one call (8192 items on the persistent grid: several per work slot):
    bit-equal to the per-channel call on channels 0, 37, 127; there |Z S Z^T - I| < 1e-9 and residual < 1e-12 lambda_max
    (the bars of test_eigvecs_block_vs_lapack)."""
    prob, SB, HB, E = c4
    count = 64
    Z = prob.eigvecs_batch(0, 128, 1, count)
    for l in (0, 37, 127):
        assert np.array_equal(Z[l], prob.eigvecs(l, 1, count)), l
        SZ = band_mv(SB, Z[l].T)
        G = Z[l] @ SZ
        assert np.max(np.abs(G - np.eye(count))) < 1e-9, l
        lam = np.max(np.abs(E[l]))
        res = np.max(np.abs(band_mv(HB[l], Z[l].T) - SZ * E[l, :count][None, :])) / lam
        assert res < 1e-12, (l, res)


def test_eigvecs_batch_all_vectors_rate(c4):
    """All 4096 vectors of 32 channels through the _dev variant, against bspatom_eigvecs per channel (2 channels) in the
    same process: bit-equal there, and less time per channel."""
    prob, _, _, _ = c4
    n, nl, loop_ch = prob.nfun, 32, 2
    Zd = torch.empty((nl, n, n), dtype=torch.float64, device="cuda:0")
    prob.eigvecs_batch_dev(0, 1, 1, 1, Zd.data_ptr())            # first launch of the kernel outside the timing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prob.eigvecs_batch_dev(0, nl, 1, n, Zd.data_ptr())           # returns when the vectors are there
    torch.cuda.synchronize()
    t_batch = (time.perf_counter() - t0) / nl
    t0 = time.perf_counter()
    R = [prob.eigvecs(l, 1, n) for l in range(loop_ch)]
    t_loop = (time.perf_counter() - t0) / loop_ch
    for l in range(loop_ch):
        assert np.array_equal(Zd[l].cpu().numpy(), R[l]), l
    note("eigvecs_batch C4 all vectors: %.1f channels/s (%.1f ms per channel, 32 channels, _dev); per-channel loop %.1f channels/s "
         "(%.1f ms); x%.1f" % (1.0 / t_batch, 1e3 * t_batch, 1.0 / t_loop, 1e3 * t_loop, t_loop / t_batch))
    assert t_batch < t_loop, (t_batch, t_loop)


class _PerChannelOnly:
    """a problem that exposes eigvecs only: write_eigenvec_all takes its per-channel path"""

    def __init__(self, prob):
        self.nfun = prob.nfun
        self.eigvecs = prob.eigvecs


@pytest.mark.parametrize("name", ["pi3_emax1", "pi3_nobound"])
def test_eigenvec_all_unchanged_through_the_batch(tmp_path, name):
    """Eigenvec_All.dat byte for byte the same through eigvecs_batch and through eigvecs per channel, the same as host.run
    writes, and (when built) the Fortran host's file parses to the same values."""
    text = open(golden_input(name)).read()
    (tmp_path / "run").mkdir()
    host.run(text, outdir=str(tmp_path / "run"))
    ref = (tmp_path / "run" / "Eigenvec_All.dat").read_bytes()
    nfun, n1_max, lmax = (int(t) for t in ref.split(b"\n", 1)[0].split())
    prob = capi.Problem(host.input_from_namelist(text))
    assert prob.lmax == lmax
    E, info = prob.solve(0, lmax + 1)
    assert np.all(info == 0)
    pb, pc = tmp_path / "batch.dat", tmp_path / "per_channel.dat"
    host.write_eigenvec_all(str(pb), prob, lmax, n1_max)
    host.write_eigenvec_all(str(pc), _PerChannelOnly(prob), lmax, n1_max)
    prob.close()
    assert pb.read_bytes() == pc.read_bytes()
    assert pb.read_bytes() == ref
    exe = os.path.join(ROOT, "bspatom_amd", "bsp_atom_host.x")
    if os.path.exists(exe):
        (tmp_path / "f").mkdir()
        with open(golden_input(name)) as fin:
            p = subprocess.run([exe], stdin=fin, cwd=tmp_path / "f", capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        nf, n1, lm, Cf = host.read_eigenvec_all(str(tmp_path / "f" / "Eigenvec_All.dat"))
        _, _, _, Cp = host.read_eigenvec_all(str(pc))
        assert (nf, n1, lm) == (nfun, n1_max, lmax)
        assert np.array_equal(Cf, Cp)
