"""Python host of libbspatom mirroring the reference driver up to the end of SOLVE_SYSTEM
(PROGRAM BSP_ATOM_PI, src/Bsp_Atom.f90:45-95; SOLVE_SYSTEM, src/matrices.f90:204-386):
namelist text -> spectra, the (l_ini, n0_ini) eigenvector, Enl.dat / wf_n0.dat / stdout text in the
reference's formats for KIND_PI = 0, and for KIND_PI >= 3 also the state limits (`select_states`) and
Eigenvec_All.dat.  All arithmetic on matrices happens in libbspatom on the GPU; this module only parses,
dispatches, does the reference's integer bookkeeping on the spectra and formats."""
import math
import os
from fractions import Fraction as _F
from . import capi
from .namelist import read_namelists


def fortran_g(v, w, d, e=2):
    """Fortran Gw.d (e = 2) or Gw.dEe edit descriptor (F2008 10.7.5.2.2) for a real value, as gfortran/flang print it:
    F editing with e + 2 trailing blanks inside the range, else 0.dddE+xx with e exponent digits."""
    pad = " " * (e + 2)
    if v == 0.0:
        body = "%.*f" % (d - 1, 0.0)
        return (body + pad).rjust(w)
    return _fortran_g_tail(v, w, d, e, pad, abs(v))


def _fortran_g_tail(v, w, d, edig, pad, a):
    e = math.floor(math.log10(a)) + 1
    if float("%.*e" % (d - 1, a)) >= 10.0 ** e:
        e += 1
    if 0 <= e <= d:
        body = "%.*f" % (d - e, v)
        return (body + pad).rjust(w)
    m = "%.*E" % (d - 1, v)            # d.ddddE+xx -> 0.ddddd E+(xx+1)
    mant, ex = m.split("E")
    sign = "-" if mant.startswith("-") else ""
    digits = mant.replace("-", "").replace(".", "")
    ex = int(ex) + 1
    return ("%s0.%sE%+0*d" % (sign, digits, edig + 1, ex)).rjust(w)


def kind_pi_from_namelist(text):
    return int(read_namelists(text)["vars_field"].get("kind_pi", 0))


def input_from_namelist(text):
    nl = read_namelists(text)
    kw = {}
    kw.update(nl["vars_bsp"]); kw.update(nl["vars_tise"])
    return capi.make_input(**kw)


class StateLimits:
    """What the KIND_PI >= 3 branch of SOLVE_SYSTEM leaves behind: n01[l] = (n0_fin, n1_fin, nE0-1) (1-based, as
    stored), nbold[l], ntemp[l] (columns of Hij kept per channel), n1_max, nbds, emax_fin (as modified), reki."""


def select_states(E, emax_fin, kind_pi):
    """Integer bookkeeping of SOLVE_SYSTEM for KIND_PI >= 3 on the spectra E[l][i] (matrices.f90:290-341 per
    channel, :355-358 for n1_max), statement by statement, including what the reference carries over from one
    channel to the next: `Emax_fin = -1` is replaced ONCE by En(nfun) of l = 0 and later channels then use
    `Elim = Emax_fin + 0.25` (:292-298); n0_fin / n1_fin / ntemp keep the previous channel's value when no
    eigenvalue qualifies (:302-313), so a channel without bound states reports n0_fin one higher than the one
    before.  Also the density-of-states factors rEki (:333-337; 1 where the reference leaves its initial value)."""
    import numpy as np
    E = np.asarray(E, dtype=np.float64)
    nl, nfun = E.shape
    n0_fin = -1; n1_fin = -1; nlim = 0; nbds = 0
    ntemp = 0                                   # the reference leaves it undefined until an eigenvalue <= Elim is seen
    out = StateLimits()
    out.n01 = np.zeros((nl, 3), dtype=np.int64); out.nbold = []; out.ntemp = []
    out.reki = np.ones((nl, nfun))
    for l in range(nl):
        En = E[l]
        if emax_fin == -1.0:
            emax_fin = float(En[nfun - 1]); elim = emax_fin
        else:
            elim = emax_fin + 0.25
            if kind_pi >= 8:
                elim = emax_fin
        i = 1; nbold = 0
        while True:
            e = En[i - 1]
            if e < 0.0:
                n0_fin = i; nbold += 1
            if e <= emax_fin:
                n1_fin = i
            if e <= elim:
                ntemp = i
            if e > emax_fin and e > elim:
                break
            i += 1
            if i > nfun:
                break
        nbds = max(nbds, nbold)
        n0_fin += 1; n1_fin += 1
        ne0 = n0_fin
        if kind_pi >= 5:
            n0_fin = 1
        nlim = max(nlim, ntemp)
        out.n01[l] = (n0_fin, n1_fin, ne0 - 1)
        out.nbold.append(nbold)
        ntemp = min(max(n1_fin + 40, nlim), nfun)
        out.ntemp.append(ntemp)
        # density of states: rEki(i) = sqrt(2/(E(i+1)-E(i-1))) inside, one-sided at nE0 and nfun
        if not 1 <= ne0 < nfun:
            raise ValueError("no continuum state in channel l=%d (the reference indexes En(%d) here)" % (l, ne0 + 1))
        for i in range(ne0 + 1, nfun):
            out.reki[l, i - 1] = math.sqrt(2.0 / (En[i] - En[i - 2]))
        out.reki[l, ne0 - 1] = math.sqrt(1.0 / (En[ne0] - En[ne0 - 1]))
        out.reki[l, nfun - 1] = math.sqrt(1.0 / (En[nfun - 1] - En[nfun - 2]))
    out.n1_max = min(max(int(out.n01[:, 1].max()) + 20, nlim), nfun)
    out.nbds = nbds; out.emax_fin = emax_fin
    if out.n1_max > out.ntemp[0]:
        # ctemp is allocated once, at l = 0, with ntemp(l=0) columns (:321-325): the reference would read past it
        raise ValueError("n1_max = %d exceeds the %d vectors the reference keeps (ctemp, matrices.f90:321)" % (out.n1_max, out.ntemp[0]))
    return out


def run(text, outdir=".", device=0, npts=10000):
    """`Bsp_Atom_omp.x < bsp_0.inp` on the MI355X: returns (E[lmax+1, nfun], c, stdout_text)."""
    inp = input_from_namelist(text)
    kind_pi = kind_pi_from_namelist(text)
    prob = capi.Problem(inp, device)
    out = ["PROGRAM TO CALCULATE ELECTRONIC STRUCTURE AND PI CROSS SECTIONS,".rjust(64), "  USING B-SPLINES", ""]
    out.append("Number of B-spline Functions / l: nfun =%5d" % prob.nfun)
    out.append("\nMax. Angular Momenta Included: l_max =%3d" % prob.lmax)
    E, info = prob.solve(0, prob.lmax + 1)
    c = None
    lim = None
    if kind_pi >= 3 and not any(info):
        lim = select_states(E, inp.emax_fin, kind_pi)
    with open(os.path.join(outdir, "Enl.dat"), "w") as f:
        f.write(" %d\n" % prob.nfun)                                   # WRITE(75,*) nfun
        for l in range(prob.lmax + 1):
            if info[l] != 0:
                out.append(" ERROR DIAGONALIZING THE MATRIX! %d" % info[l])
                out.append("\n l = %2d" % l)
                raise RuntimeError("\n".join(out[-2:]))
            out.append("\n l0 = %2d" % l)
            out.append(" HC = ESC eigenvalue solved\n")
            out.append("    n   Eigenvalues")
            out.append("    -   -----------")
            for i in range(prob.nfun):
                line = " %4d  %s" % (i + 1, fortran_g(E[l, i], 22, 15))      # FORMAT(T2,I4,T8,G22.15)
                if i < 20:
                    out.append(" %4d  %s" % (i + 1 + l, fortran_g(E[l, i], 22, 15)))
                f.write(line + "\n")
            if l == inp.l_ini:
                out.append("\nWriting down Initial State WF\n")
                c = prob.eigvec(l, inp.n0_ini)
                r, u = prob.write_wf(c, npts)                          # raises where the reference STOPs
                with open(os.path.join(outdir, "wf_n0.dat"), "w") as g:
                    for ri, ui in zip(r, u):
                        g.write(fortran_g(ri, 20, 10) + fortran_g(ui, 20, 10) + "\n")   # '(2G20.10)'
            if lim is not None:
                out.append("\nNUMBER OF BOUND STATES:%3d" % lim.nbold[l])                 # '(/,A23,I3)'
                out.append("LIMITS FOR l =%3d STATE%5d%5d" % (l, lim.n01[l, 0] + l, lim.n01[l, 1] + l))   # '(A14,I3,A6,2I5)'
    if lim is not None:
        out.append("n1_max =%5d" % lim.n1_max)                                          # '(A8,I5)'
        write_eigenvec_all(os.path.join(outdir, "Eigenvec_All.dat"), prob, prob.lmax, lim.n1_max)
    prob.close()
    os.makedirs(os.path.join(outdir, "CSs"), exist_ok=True)            # Bsp_Atom.f90:59-60 (`mkdir CSs` at start-up)
    if kind_pi in (1, 2):                                              # Bsp_Atom.f90:77-92: TRANS_AMP, CROSS_SECTIONS
        r = cross_sections(text, outdir=outdir, device=device)
        out.append("\n" + r["stdout"])
    if kind_pi in (0, 1, 2):
        out.append("\nProgram Finished!")          # KIND_PI >= 3 continues into the Gaussian / LG-beam branch in the reference
    return E, c, "\n".join(out)


EIGVECS_GROUP_BYTES = 256 << 20       # write_eigenvec_all: host memory for the vectors of one group of channels


def write_eigenvec_all(path, prob, lmax, n1_max):
    """`Eigenvec_All.dat` as SOLVE_SYSTEM writes it for KIND_PI >= 3 (matrices.f90:366-378): a list-directed
    header `nfun n1_max lmax`, then per channel a list-directed `l` and n1_max records FORMAT(I5,5000G20.10)
    `ni, c(1:nfun)`; the reader is READ_EIGENVEC (ReadInputs.f90:792-830).  n1_max comes from `select_states`;
    channels 0..lmax must have been solved.  List-directed integers are written the way flang does (one blank,
    no padding), which is what the golden files hold; gfortran/ifort pad them, READ(*,*) accepts either."""
    nfun = prob.nfun
    # a problem with eigvecs_batch gives the vectors of a group of channels per call (one launch instead of one per channel;
    # the same bits), at most EIGVECS_GROUP_BYTES of them at a time
    batch = getattr(prob, "eigvecs_batch", None)
    group = max(1, EIGVECS_GROUP_BYTES // (8 * max(1, n1_max * nfun)))
    Zg, g0 = None, 0
    with open(path, "w") as f:
        f.write(" %d %d %d\n" % (nfun, n1_max, lmax))                  # WRITE(80,*) nfun, n1_max, lmax
        for l in range(lmax + 1):
            f.write(" %d\n" % l)
            if batch is None:
                Z = prob.eigvecs(l, 1, n1_max)
            else:
                if Zg is None or l >= g0 + len(Zg):
                    g0 = l
                    Zg = batch(l, min(group, lmax + 1 - l), 1, n1_max)
                Z = Zg[l - g0]
            for ni in range(n1_max):
                f.write("%5d" % (ni + 1) + "".join(fortran_g(v, 20, 10) for v in Z[ni]) + "\n")


def read_eigenvec_all(path):
    """Reads the file back the way READ_EIGENVEC does: returns (nfun, n1_max, lmax, c[l][ni][i])."""
    import numpy as np
    with open(path) as f:
        nfun, n1, lmax = (int(t) for t in f.readline().split())
        c = np.zeros((lmax + 1, n1, nfun))
        for l in range(lmax + 1):
            assert int(f.readline().split()[0]) == l
            for ni in range(n1):
                line = f.readline()
                assert int(line[:5]) == ni + 1
                c[l, ni] = [float(line[5 + 20 * i: 25 + 20 * i]) for i in range(nfun)]
    return nfun, n1, lmax, c



def read_enl(path, lmax, emax_fin=-1.0):
    """Reads `Enl.dat` back the way the reference's consumers do (READ_FR, ReadInputs.f90:292-316): list-directed
    `nfun`, then (lmax+1)*nfun records `i, En`; returns (nfun, Enl[l][i], n01[l]) with n01 = (1, n1_fin, n0_fin) as
    that reader rebuilds it (last index with En <= Emax_fin, last index with En < 0, both carried over between
    channels and starting undefined in the reference: 0 here)."""
    import numpy as np
    with open(path) as f:
        nfun = int(f.readline().split()[0])
        E = np.zeros((lmax + 1, nfun)); n01 = np.zeros((lmax + 1, 3), dtype=np.int64)
        n0_fin = 0; n1_fin = 0
        for l in range(lmax + 1):
            for ni in range(1, nfun + 1):
                t = f.readline().replace(",", " ").split()
                if len(t) < 2:
                    raise ValueError("Error Reading Energies")
                e = float(t[1].replace("D", "E").replace("d", "e"))
                E[l, ni - 1] = e
                if e < 0.0:
                    n0_fin = ni
                if e <= emax_fin:
                    n1_fin = ni
            n01[l] = (1, n1_fin, n0_fin)
    return nfun, E, n01


# ---- KIND_PI = 1, 2: transition amplitudes of the one-photon (plane wave) branches ---------------------------------
def three_j(j1, j2, j3, m1, m2, m3):
    """Wigner 3j symbol, integer arguments: Racah's sum evaluated through log-factorials with the smallest exponent
    taken out (what THREE_J does, Funs_WignerSymbols.for:1-62, so that the two agree to rounding)."""
    if m1 + m2 + m3 != 0:
        return 0.0
    lf = [0.0]
    for i in range(1, j1 + j2 + j3 + 2):
        lf.append(lf[-1] + math.log(float(i)))          # lf[i] = log(i!)
    zmin = max(0, j2 - j3 - m1, j1 + m2 - j3)
    zmax = min(j1 + j2 - j3, j1 - m1, j2 + m2)
    if zmax < zmin:
        return 0.0
    delta = 0.5 * (lf[j1 + j2 - j3] + lf[j3 + j1 - j2] + lf[j3 + j2 - j1] - lf[j1 + j2 + j3 + 1]
                   + lf[j1 + m1] + lf[j1 - m1] + lf[j2 + m2] + lf[j2 - m2] + lf[j3 + m3] + lf[j3 - m3])
    ex = [lf[z] + lf[j1 + j2 - j3 - z] + lf[j1 - m1 - z] + lf[j2 + m2 - z] + lf[j3 - j2 + m1 + z] + lf[j3 - j1 - m2 + z]
          for z in range(zmin, zmax + 1)]
    g = min(min(ex), 250.0)
    acc = 0.0
    for z, e in zip(range(zmin, zmax + 1), ex):
        acc += (-1.0) ** z * math.exp(-(e - g))
    return (-1.0) ** (j1 - j2 - m3) * math.exp(delta - g) * acc


def final_channels(kind_pi, l0, m0):
    """(l, m) of the final states SEL_LM selects for the dipolar cases (grid.f90:128-143): l0-1 (if it exists and can
    carry m0) and l0+1, m unchanged; TRANS_AMP uses the LAST of them."""
    out = []
    for lf in (l0 - 1, l0 + 1):
        if lf >= 0 and lf >= m0:
            out.append((lf, m0))
    return out


def final_state_limits(E_fin, emax_fin):
    """n0_fin, n1_fin (1-based) of SOLVE_SYSTEM for KIND_PI = 1, 2 at l = l_fin (matrices.f90:272-283) and the
    Emax_fin it then uses (-1 means the largest eigenvalue)."""
    n = len(E_fin)
    if emax_fin == -1.0:
        emax_fin = float(E_fin[n - 1])
    n0 = -1; n1 = -1
    for i in range(1, n + 1):
        if E_fin[i - 1] < 0.0:
            n0 = i
        if E_fin[i - 1] <= emax_fin:
            n1 = i
    return min(n0 + 1, n - 1), n1, emax_fin


def trans_amp(text, device=0):
    """`Bsp_Atom.x < input` with KIND_PI = 1 (length gauge) or 2 (velocity gauge) up to the end of TRANS_AMP
    (Bsp_Atom.f90:72-80; PhotoIon.f90:1-107): spectra of l = 0 .. lmax on the MI355X, the final-state window, and
    T_fi(n) = An c0 <c_fin(n)| c1 rij1 + c2 rij2 |c_ini> with the dipole matrices of the same assembly pass.
    Returns dict(E, l_fin, m_fin, n0_fin, n1_fin, T_fi, stdout).  The eigenvectors carry this library's sign
    convention (LAPACK's is arbitrary), so T_fi(n) agrees with the reference up to the sign of each state.
    CROSS_SECTIONS is not reproduced: the reference computes there with Enl(n0,l0), which it allocates for
    KIND_PI >= 3 only (PhotoIon.f90:302)."""
    import numpy as np
    nl = read_namelists(text)
    kind_pi = int(nl["vars_field"].get("kind_pi", 0))
    if kind_pi not in (1, 2):
        raise ValueError("trans_amp: KIND_PI must be 1 or 2")
    mph = int(nl["vars_field"].get("mph", 0))
    kw = {}
    kw.update(nl["vars_bsp"]); kw.update(nl["vars_tise"])
    inp = capi.make_input(**kw)
    l0, m0, n0 = inp.l_ini, inp.m_ini, inp.n0_ini
    lf, mf = final_channels(kind_pi, l0, m0)[-1]
    prob = capi.Problem(inp, device)
    if lf > prob.lmax:
        prob.close()
        raise ValueError("l_fin = l_ini + 1 = %d is beyond lmax = %d of the input (the reference reads an unallocated "
                         "ci_fin in that case)" % (lf, prob.lmax))
    E, info = prob.solve(0, prob.lmax + 1)
    if any(info):
        prob.close()
        raise RuntimeError("ERROR DIAGONALIZING THE MATRIX! %s" % list(info))
    n0f, n1f, _ = final_state_limits(E[lf], inp.emax_fin)
    if n1f + 1 > prob.nfun:
        prob.close()
        raise ValueError("n1_fin = nfun: the density-of-states factor needs E_fin(n1_fin + 1)")
    t3a = three_j(lf, 1, l0, -mf, mph, m0)
    if kind_pi == 1:
        t3b = three_j(lf, 1, l0, 0, 0, 0)
        c1 = (-1.0) ** (lf + l0 + mf) * math.sqrt(float((2 * lf + 1) * (2 * l0 + 1))) * t3a * t3b
        c0 = 1.0
        a = [c1, 0.0, 0.0]                                         # A = c1 * int B r B
    else:
        c0 = math.sqrt(float(l0 + 1)) * t3a
        c1, c2 = (float(l0 + 1), -1.0) if lf == l0 + 1 else ((float(l0), 1.0) if lf == l0 - 1 else (0.0, 0.0))
        a = [0.0, c1, c2]                                          # A = c1 * int B B / r + c2 * int B B'
    D = prob.dipole_elements(l0, n0, lf, n0f, n1f - n0f + 1, a)
    Ef = E[lf]
    T = np.array([math.sqrt(2.0 / (Ef[ni] - Ef[ni - 2])) * c0 * D[ni - n0f] for ni in range(n0f, n1f + 1)])
    out = ["LIMITS FOR FINAL STATE (l=%2d) : %4d%4d" % (lf, n0f, n1f),                 # '(/,A26,I2,A3,X,2I4)'
           "Calculating Transition Amplitudes",
           "Initial State:%3d%3d%3d" % (n0 + l0, l0, m0)]                              # '(A14,3I3)'
    prob.close()
    return dict(E=E, l_fin=lf, m_fin=mf, n0_fin=n0f, n1_fin=n1f, T_fi=T, stdout="\n".join(out))


# a.u. -> Mb and the speed of light of the reference (Modules.f90:12)
C_AU = 137.03599913815
A_AU = 5.29177249e-9


def cross_sections(text, outdir=".", device=0):
    """KIND_PI = 1, 2 to the end of CROSS_SECTIONS (PhotoIon.f90:274-468): `CSs/CrossSection_Len.dat` (length gauge) or
    `CSs/CrossSection_Vel.dat` (velocity gauge), one record FORMAT(2G20.10E3) `E_fin(nf), sigma(nf)` per final state
    nf = n0_fin .. n1_fin, sigma = M_au c0 c1 d1 T_fi(nf)^2 with M_au = a_au^2 1e18 (Mb), c0 = 4 pi^2 / c_au,
    c1 = 1/(2 l0 + 1), d1 = E_fin(nf) - E_ini(n0) (length) or its reciprocal (velocity) (:316-322, :387-394, :403).
    Two deviations from the reference AS WRITTEN, both where it reads variables SOLVE_SYSTEM sets for KIND_PI >= 3
    only: the loop `DO nf = n0_fin, n1_max` (:385) runs to n1_fin (the records are written for nf <= n1_fin anyway,
    :408), and the printed `E0=` (:302-303, Enl(n0,l0): unallocated here) is E_ini(n0).  The fixtures
    tests/golden/cs_*.npz come from the reference's own routine called with those two values set by the dump driver.
    T_fi is squared, so the arbitrary eigenvector signs drop out."""
    r = trans_amp(text, device=device)
    nl = read_namelists(text)
    kind_pi = int(nl["vars_field"]["kind_pi"])
    n0 = int(nl["vars_tise"].get("n0_ini", 1)); l0 = int(nl["vars_tise"].get("l_ini", 0))
    E_ini = r["E"][l0]; E_fin = r["E"][r["l_fin"]]
    m_au = (A_AU ** 2) * 1.0e18
    c0 = 4.0 * (math.pi ** 2) / C_AU
    c1 = 1.0 / float(2 * l0 + 1)
    rows = []
    for nf in range(r["n0_fin"], r["n1_fin"] + 1):
        d1 = E_fin[nf - 1] - E_ini[n0 - 1]
        if kind_pi == 2:
            d1 = 1.0 / d1
        d2 = r["T_fi"][nf - r["n0_fin"]] ** 2
        rows.append((E_fin[nf - 1], m_au * c0 * c1 * d1 * d2))
    os.makedirs(os.path.join(outdir, "CSs"), exist_ok=True)
    name = "CrossSection_Len.dat" if kind_pi == 1 else "CrossSection_Vel.dat"
    with open(os.path.join(outdir, "CSs", name), "w") as f:
        for ef, cs in rows:
            f.write(fortran_g(ef, 20, 10, 3) + fortran_g(cs, 20, 10, 3) + "\n")
    r["rows"] = rows
    r["file"] = os.path.join("CSs", name)
    r["stdout"] = r["stdout"] + "\n\nCalculating Cross Sections\n E0= %s" % repr(float(E_ini[n0 - 1]))
    return r


# ---- CSs/MatElem_All.dat: the coupling file the sibling TDSE tools read ------------------------------
def write_matelem_all(path, n1_max, zT):
    """`CSs/MatElem_All.dat` as TRANS_AMP writes it (PhotoIon.f90:255-266): list-directed header `n1_max nbra nket`, then
    for ibra = 1..nbra, jket = ibra..nket one record FORMAT(2I8,X,20G20.10) `ibra, jket, (Re, Im of zT(ibra,jket,i),
    i = 1..ncomp)`.  zT: complex array (nbra, nket, ncomp), upper triangle used.  The reader is READ_COUP
    (ReadInputs.f90:324-366)."""
    nbra, nket, ncomp = zT.shape
    with open(path, "w") as f:
        f.write(" %d %d %d\n" % (n1_max, nbra, nket))
        for ib in range(nbra):
            for jk in range(ib, nket):
                rec = "%8d%8d " % (ib + 1, jk + 1)
                for i in range(ncomp):
                    z = complex(zT[ib, jk, i])
                    rec += fortran_g(z.real, 20, 10) + fortran_g(z.imag, 20, 10)
                f.write(rec + "\n")


def read_matelem_all(path, nfields=1):
    """Reads the file back the way READ_COUP does (ReadInputs.f90:324-366): list-directed `n1_max nbra nket`, then
    list-directed records `ibra jket f(1:2 nfields)`; returns (n1_max, zHint[nbra][nket][nfields]), upper triangle."""
    import numpy as np
    with open(path) as f:
        n1_max, nbra, nket = (int(t) for t in f.readline().split())
        z = np.zeros((nbra, nket, nfields), dtype=np.complex128)
        for ni in range(nbra):
            for nj in range(ni, nket):
                t = f.readline().replace(",", " ").split()
                if len(t) < 2 + 2 * nfields:
                    raise ValueError("Error Reading Couplings File")
                ib, jk = int(t[0]), int(t[1])
                v = [float(x.replace("D", "E")) for x in t[2: 2 + 2 * nfields]]
                for i in range(nfields):
                    z[ib - 1, jk - 1, i] = complex(v[2 * i], v[2 * i + 1])
    return n1_max, z


def dipole_blocks(channels, kind_pi=1, mph=0):
    """The nonzero blocks of the one-photon dipole coupling between `channels` (a list of (l, m)), upper triangle: a list of
    (a_, b_, l0, lf, c0, coef) with a_ <= b_ the positions of the bra and the ket channel, l0 = l of the ket (initial), lf = l of
    the bra (final), and the reference's angular factors (PhotoIon.f90:66-83): the block is c0 * <lf| coef . (r, 1/r, d/dr) |l0>."""
    blocks = []                                    # (a_, b_, initial channel, final channel, c0, coefficients)
    for a_, (li, mi) in enumerate(channels):
        for b_, (lj, mj) in enumerate(channels):
            if abs(li - lj) != 1 or b_ < a_:
                continue
            # <bra = (li, mi)| A |ket = (lj, mj)>: the reference's c0, c1, c2 with l0 = lj (initial), lf = li (final)
            l0, m0, lf, mf = lj, mj, li, mi
            t3a = three_j(lf, 1, l0, -mf, mph, m0)
            if kind_pi == 1:
                t3b = three_j(lf, 1, l0, 0, 0, 0)
                c1 = (-1.0) ** (lf + l0 + mf) * math.sqrt(float((2 * lf + 1) * (2 * l0 + 1))) * t3a * t3b
                c0 = 1.0; coef = [c1, 0.0, 0.0]
            else:
                c0 = math.sqrt(float(l0 + 1)) * t3a
                c1, c2 = (float(l0 + 1), -1.0) if lf == l0 + 1 else (float(l0), 1.0)
                coef = [0.0, c1, c2]
            blocks.append((a_, b_, l0, lf, c0, coef))
    return blocks


def dipole_matelem(prob, channels, n1_max, kind_pi=1, mph=0):
    """Coupling matrix of the one-photon dipole operator between the states (l, n = 1..n1_max) of `channels` (a list of
    (l, m)), laid out as TRANS_AMP lays out zT_fi for the beam cases: row / column index = il * n1_max + n (il = position
    in `channels`), one component.  <n l m| c1 r |n' l' m'> in the length gauge (KIND_PI = 1) or the velocity-gauge
    operator (KIND_PI = 2) with the angular factors of PhotoIon.f90:66-83; zero unless l' = l +- 1.  The reference
    writes MatElem_All.dat only for its Gaussian / LG-beam branches (angular integrals outside SURVEY 8); this fills
    the same file with the plane-wave couplings so that READ_COUP consumers can run on the GPU solver's output."""
    import numpy as np
    nlm = len(channels)
    z = np.zeros((nlm * n1_max, nlm * n1_max, 1), dtype=np.complex128)
    blocks = dipole_blocks(channels, kind_pi, mph)
    if hasattr(prob, "dipole_matrix") and blocks:
        # every block of the file in one call (bspatom_dipole_matrix): D[p][nj - 1][n - 1], ket = initial, bra = final
        D = prob.dipole_matrix([(l0, lf) for _, _, l0, lf, _, _ in blocks], 1, n1_max, 1, n1_max,
                               np.array([coef for *_, coef in blocks], dtype=np.float64))
        for p, (a_, b_, _, _, c0, _) in enumerate(blocks):
            z[a_ * n1_max: (a_ + 1) * n1_max, b_ * n1_max: (b_ + 1) * n1_max, 0] = c0 * D[p].T
        return z
    for a_, b_, l0, lf, c0, coef in blocks:
        for nj in range(1, n1_max + 1):
            D = prob.dipole_elements(l0, nj, lf, 1, n1_max, coef)
            z[a_ * n1_max: (a_ + 1) * n1_max, b_ * n1_max + nj - 1, 0] = c0 * D
    return z


# ---- the TDSE in the eigenstate basis (Problem.tdse_propagate): tableau, field table, couplings, CSs/TDSE_COEFFs.dat --------
# MOD_RK_PARAMS (Modules.f90:559-586) as exact fractions: a21 .. a65 (:568-572), b (:574-575, b6 = 0), c (:577-578), d (:580-581)
RK_A = ((), (_F(2, 9),), (_F(1, 12), _F(1, 4)), (_F(69, 128), _F(-243, 128), _F(135, 64)),
        (_F(-17, 12), _F(27, 4), _F(-27, 5), _F(16, 15)), (_F(65, 432), _F(-5, 16), _F(13, 16), _F(4, 27), _F(5, 144)))
RK_B = (_F(1, 9), _F(0), _F(9, 20), _F(16, 45), _F(1, 12), _F(0))
RK_C = (_F(0), _F(2, 9), _F(1, 3), _F(3, 4), _F(1), _F(5, 6))
RK_D = (_F(47, 450), _F(0), _F(12, 25), _F(32, 225), _F(1, 30), _F(6, 25))


def rk_nodes(t0, dt, nsteps):
    """The (nsteps, 6) stage times t0 + (n + c_s) dt of Problem.tdse_propagate."""
    import numpy as np
    c = np.array([float(x) for x in RK_C])
    return float(t0) + (np.arange(nsteps, dtype=np.float64)[:, None] + c[None, :]) * float(dt)


def field_table(fns, t0, dt, nsteps):
    """The field argument of Problem.tdse_propagate: complex (nsteps, 6, nscan), [n, s, q] = f_q(t0 + (n + c_s) dt).  fns: one entry
    per scan, a callable of the array of times or an array of shape (nsteps, 6) already on rk_nodes(t0, dt, nsteps)."""
    import numpy as np
    t = rk_nodes(t0, dt, nsteps)
    fns = list(fns)
    out = np.zeros((nsteps, 6, len(fns)), dtype=np.complex128)
    for q, f in enumerate(fns):
        v = np.asarray(f(t) if callable(f) else f, dtype=np.complex128)
        if v.shape != t.shape:
            raise ValueError("scan %d: the field must give one value per stage time %s, got shape %s" % (q, t.shape, v.shape))
        out[:, :, q] = v
    return out


def field_nodes(fns, dfns, t0, dt, nsteps, nsub):
    """The fn argument of Problem.tdse_adaptive: complex (nsteps * nsub + 1, 2, nscan), [i, 0, q] = f_q and [i, 1, q] = df_q/dt at the
    nodes t0 + i dt / nsub.  fns: one callable of the array of times per scan; dfns: their time derivatives, or None: then the
    derivative is the centred difference (f(t + d) - f(t - d)) / (2 d) with d = hf / 8, hf = dt / nsub the node spacing (its error is
    O(hf^2) times the third derivative, O(hf^3) in the interpolated field; give dfns where that matters)."""
    import numpy as np
    if nsteps < 0 or nsub < 1:
        raise ValueError("field_nodes needs nsteps >= 0 and nsub >= 1")
    hf = float(dt) / nsub
    t = float(t0) + np.arange(nsteps * nsub + 1, dtype=np.float64) * hf
    fns = list(fns)
    dfns = None if dfns is None else list(dfns)
    if dfns is not None and len(dfns) != len(fns):
        raise ValueError("field_nodes: %d fields but %d derivatives" % (len(fns), len(dfns)))
    out = np.zeros((len(t), 2, len(fns)), dtype=np.complex128)
    d = hf / 8.0
    for q, f in enumerate(fns):
        out[:, 0, q] = np.asarray(f(t), dtype=np.complex128)
        if dfns is None:
            out[:, 1, q] = (np.asarray(f(t + d), dtype=np.complex128) - np.asarray(f(t - d), dtype=np.complex128)) / (2.0 * d)
        else:
            out[:, 1, q] = np.asarray(dfns[q](t), dtype=np.complex128)
    return out


def adapt_steps(log_i, t0, dt):
    """The accepted steps of the log of Problem.tdse_adaptive: (t, h), the start time t0 + dt (n + j / 2^m) and the size dt / 2^m of
    every attempt with flag 1 or 2 in log_i (nlog, 4) rows (n, m, j, flag), in order."""
    import numpy as np
    li = np.asarray(log_i, dtype=np.int64).reshape(-1, 4)
    li = li[li[:, 3] > 0]
    n, m, j = li[:, 0], li[:, 1].astype(np.int32), li[:, 2]
    t = float(t0) + float(dt) * (n.astype(np.float64) + np.ldexp(j.astype(np.float64), -m))
    return t, np.ldexp(np.full(len(li), float(dt)), -m)


def obs_steps(nsteps, obs_every):
    """The step numbers n_j of the rows of Problem.tdse_observe: 0, obs_every, 2 obs_every, .. < nsteps, then nsteps; row j
    describes a(t0 + n_j dt).  nsteps = 0: the one row [0]."""
    if nsteps < 0 or obs_every < 1:
        raise ValueError("obs_steps needs nsteps >= 0 and obs_every >= 1")
    return [0] if nsteps == 0 else list(range(0, nsteps, obs_every)) + [nsteps]


def tdse_expectations(obs):
    """(norm, <H0>, 2 Re z, 2 Im z), each (nobs, nscan), of the rows obs (nobs, nscan, nch, 4) of Problem.tdse_observe: the sums over
    the channels of pop, sum E |a|^2 and z_c.  <H_int> = 2 Re(f z); length gauge: <D> = 2 Re z; velocity gauge (f = -i A on the
    real blocks): 2 Im z."""
    import numpy as np
    s = np.asarray(obs, dtype=np.float64).sum(axis=-2)
    return s[..., 0], s[..., 1], 2.0 * s[..., 2], 2.0 * s[..., 3]


def tdse_system(prob, channels, n0, count, kind_pi=1, mph=0):
    """(E, pairs, D) of Problem.tdse_propagate for the states n0 .. n0+count-1 (1-based) of `channels`, a list of (l, m) of the
    last solve: E (nch, count) from that solve, pairs = positions (ket channel, bra channel) of dipole_blocks, D (npairs, count,
    count) = c0 * dipole_matrix in ONE call -- the blocks dipole_matelem writes to MatElem_All.dat, D[p, i, f] = z[bra f, ket i].
    Length gauge (kind_pi = 1): drive with f = F(t); velocity gauge (2): with f = -i A(t)."""
    import numpy as np
    E_all, l_first = getattr(prob, "last_E", None), getattr(prob, "last_l0", 0)
    if E_all is None:
        raise ValueError("tdse_system needs the eigenvalues of the problem's last solve()")
    E = np.stack([np.asarray(E_all[l - l_first][n0 - 1: n0 - 1 + count], dtype=np.float64) for l, _ in channels])
    if E.shape != (len(channels), count):
        raise ValueError("states %d .. %d are not in the last solve" % (n0, n0 + count - 1))
    blocks = dipole_blocks(channels, kind_pi, mph)
    pairs = [(b_, a_) for a_, b_, *_ in blocks]
    if not blocks:
        return E, pairs, np.zeros((0, count, count))
    D = prob.dipole_matrix([(l0, lf) for _, _, l0, lf, _, _ in blocks], n0, count, n0, count,
                           np.array([coef for *_, coef in blocks], dtype=np.float64))
    D = np.array([c0 for *_, c0, _ in blocks], dtype=np.float64)[:, None, None] * D
    return E, pairs, D


def dipole_blocks_pol(channels):
    """The length-gauge blocks of a field of any direction between `channels` (a list of (l, m)), for Problem.tdse_fields: (blocks,
    fidx), blocks as dipole_blocks gives them.  First the nonzero q = 0 blocks of dipole_blocks(channels, 1, 0), on field 0; then the
    q = +1 blocks on field 1, for EVERY ordered (bra, ket) pair of channels whose 3j symbol is nonzero (m_bra = m_ket + 1): r_{+1} is
    not Hermitian, and the conjugate partner the call gives every pair supplies -r_{-1}.  The angular factor is dipole_blocks'."""
    blocks = [b for b in dipole_blocks(channels, 1, 0) if b[5][0] != 0.0]          # dipole_blocks keeps the pairs whose 3j symbol vanishes
    fidx = [0] * len(blocks)
    for a_, (li, mi) in enumerate(channels):
        for b_, (lj, mj) in enumerate(channels):
            if abs(li - lj) != 1:
                continue
            l0, m0, lf, mf = lj, mj, li, mi
            t3a = three_j(lf, 1, l0, -mf, 1, m0)
            if t3a == 0.0:
                continue
            t3b = three_j(lf, 1, l0, 0, 0, 0)
            c1 = (-1.0) ** (lf + l0 + mf) * math.sqrt(float((2 * lf + 1) * (2 * l0 + 1))) * t3a * t3b
            blocks.append((a_, b_, l0, lf, 1.0, [c1, 0.0, 0.0]))
            fidx.append(1)
    return blocks, fidx


def tdse_system_pol(prob, channels, n0, count):
    """(E, pairs, D, fidx) of Problem.tdse_fields for the states n0 .. n0+count-1 (1-based) of `channels`, a list of (l, m) of the last
    solve, in the length gauge under a field of any direction: tdse_system's E, the blocks of dipole_blocks_pol from ONE
    dipole_matrix call, fidx[p] = 0 (r_0, driven by f_0 = F_z) or 1 (r_{+1}, driven by f_1 = -(F_x - i F_y) / sqrt 2): field_table_pol."""
    import numpy as np
    E_all, l_first = getattr(prob, "last_E", None), getattr(prob, "last_l0", 0)
    if E_all is None:
        raise ValueError("tdse_system_pol needs the eigenvalues of the problem's last solve()")
    E = np.stack([np.asarray(E_all[l - l_first][n0 - 1: n0 - 1 + count], dtype=np.float64) for l, _ in channels])
    if E.shape != (len(channels), count):
        raise ValueError("states %d .. %d are not in the last solve" % (n0, n0 + count - 1))
    blocks, fidx = dipole_blocks_pol(channels)
    pairs = [(b_, a_) for a_, b_, *_ in blocks]
    if not blocks:
        return E, pairs, np.zeros((0, count, count)), fidx
    D = prob.dipole_matrix([(l0, lf) for _, _, l0, lf, _, _ in blocks], n0, count, n0, count,
                           np.array([coef for *_, coef in blocks], dtype=np.float64))
    D = np.array([c0 for *_, c0, _ in blocks], dtype=np.float64)[:, None, None] * D
    return E, pairs, D, fidx


def field_table_pol(F, t0, dt, nsteps):
    """The field argument of Problem.tdse_fields for the blocks of dipole_blocks_pol: complex (nsteps, 6, 2, nscan) with f_0 = F_z and
    f_1 = -(F_x - i F_y) / sqrt 2 at the stage times, so that f_0 r_0 + f_1 r_{+1} + h.c. = F . r.  F: one entry per scan, a callable
    of the array of times that returns (F_x, F_y, F_z), or an array (3, nsteps, 6) on rk_nodes(t0, dt, nsteps)."""
    import numpy as np
    t = rk_nodes(t0, dt, nsteps)
    F = list(F)
    out = np.zeros((nsteps, 6, 2, len(F)), dtype=np.complex128)
    for q, f in enumerate(F):
        v = f(t) if callable(f) else f
        if len(v) != 3:
            raise ValueError("scan %d: the field must give (Fx, Fy, Fz), got %d components" % (q, len(v)))
        v = np.stack([np.broadcast_to(np.asarray(c, dtype=np.float64), t.shape) for c in v])
        out[:, :, 0, q] = v[2]
        out[:, :, 1, q] = -(v[0] - 1j * v[1]) / math.sqrt(2.0)
    return out


def tdse_dipole_vector(obs):
    """(<x>, <y>, <z>), shape (nobs, nscan, 3), from the rows obs (nobs, nscan, nch, 8) of a Problem.tdse_fields run on the blocks of
    dipole_blocks_pol: with z_g summed over the channels, <z> = 2 Re z_0, <x> = -sqrt 2 Re z_1, <y> = -sqrt 2 Im z_1 (z_1 = <r_{+1}>,
    r_{+1} = -(x + i y) / sqrt 2)."""
    import numpy as np
    obs = np.asarray(obs)
    if obs.ndim < 2 or obs.shape[-1] < 8:
        raise ValueError("tdse_dipole_vector needs the rows of tdse_fields with two fields, (.., nch, 8), got shape %s" % (obs.shape,))
    s = obs.sum(axis=-2)
    r2 = np.sqrt(s.dtype.type(2))                           # in the rows' own precision
    return np.stack([-r2 * s[..., 6], -r2 * s[..., 7], 2 * s[..., 2]], axis=-1)


def cap_profile(r, r0, eta, power=2):
    """The complex absorbing potential's W(r) = eta (r - r0)^power beyond r0, 0 inside (the Hamiltonian gains -i W(r))."""
    import numpy as np
    r = np.asarray(r, dtype=np.float64)
    return float(eta) * np.where(r > r0, r - r0, 0.0) ** power


def tdse_absorber(prob, channels, n0, count, g):
    """The static argument (spairs, skind, W) of Problem.tdse_static for an absorber -i g(r) on the states n0 .. n0+count-1 (1-based)
    of `channels`, the list of (l, m) given to tdse_system: one in-channel block of kind 1 per channel, W[c, i, f] = <f| g |i>, from
    ONE operator_matrix call.  g: a callable of the array of points or an array on the quadrature grid (cap_profile)."""
    import numpy as np
    W = operator_matrix(prob, [(l, l) for l, _ in channels], [(g, False)], n0, count, n0, count)
    nch = len(channels)
    return [(c, c) for c in range(nch)], np.ones(nch, dtype=np.int32), W


def tdse_static_rates(obs):
    """d pop_c/dt from the static blocks, 2 Im s_c, (nobs, nscan, nch), of the rows obs (nobs, nscan, nch, 6) of Problem.tdse_static;
    for a symmetric in-channel absorber that is -2 <W>_c."""
    import numpy as np
    obs = np.asarray(obs, dtype=np.float64)
    if obs.ndim != 4 or obs.shape[-1] != 6:
        raise ValueError("tdse_static_rates needs the rows of tdse_static, (nobs, nscan, nch, 6), got shape %s" % (obs.shape,))
    return 2.0 * obs[..., 5]


def tdse_yield(obs, dt, nsteps, obs_every):
    """The population the static blocks removed from each channel during the run, (nscan, nch): the integral of -2 Im s_c over the
    uniform time grid of the rows (trapezoid, spacing obs_every dt).  With an absorber, the ionisation yield per channel; yield.sum(-1)
    + norm(T) = norm(0) up to the quadrature error.  The rows form a uniform grid only when obs_every divides nsteps."""
    import numpy as np
    if obs_every < 1 or nsteps < 0:
        raise ValueError("tdse_yield needs nsteps >= 0 and obs_every >= 1")
    if nsteps % obs_every:
        raise ValueError("tdse_yield needs rows on a uniform grid: obs_every = %d does not divide nsteps = %d" % (obs_every, nsteps))
    rate = -tdse_static_rates(obs)
    if rate.shape[0] != nsteps // obs_every + 1:
        raise ValueError("%d rows do not belong to nsteps = %d, obs_every = %d" % (rate.shape[0], nsteps, obs_every))
    h = float(dt) * obs_every
    return h * (rate.sum(axis=0) - 0.5 * (rate[0] + rate[-1]))


def write_tdse_coeffs(path, a):
    """`CSs/TDSE_COEFFs.dat` as READ_TDCOEFF reads it (ReadInputs.f90:453-467): one list-directed record `n Re Im` per state, in the
    row order of MatElem_All.dat (channel position * count + n); a: complex (nch, count) or (nvec,); 17 significant digits, so
    read_tdse_coeffs returns the same bits.  n is the state's number in its channel (the reader overwrites it, :464)."""
    import numpy as np
    a = np.asarray(a, dtype=np.complex128)
    count = a.shape[-1]
    with open(path, "w") as f:
        for i, z in enumerate(a.reshape(-1)):
            f.write(" %d %.16E %.16E\n" % (i % count + 1, z.real, z.imag))


def read_tdse_coeffs(path, nvec):
    """The nvec amplitudes of `CSs/TDSE_COEFFs.dat`, read the way READ_TDCOEFF does (list-directed `ni, fi(1), fi(2)`)."""
    import numpy as np
    z = np.zeros(nvec, dtype=np.complex128)
    with open(path) as f:
        for i in range(nvec):
            t = f.readline().replace(",", " ").split()
            if len(t) < 3:
                raise ValueError("An Error Ocurred Reading the Probs: record %d" % (i + 1))
            z[i] = complex(float(t[1].replace("D", "E")), float(t[2].replace("D", "E")))
    return z


# ---- wavefunctions on r: files per state, radial integrals on the assembly's quadrature ------------------------------------
def write_wf_states(outdir, prob, l, n0, count, npts=10000):
    """One `wf_l<l>_n<n>.dat` per state n = n0 .. n0+count-1 of channel l in WRITE_WF's format (Bsp_Atom.f90:118-146:
    npts + 1 records '(2G20.10)' `r_i, u(r_i)`, r_i = ra + i*(rb-ra)/npts), all states from ONE prob.wavefunctions call.
    Returns the paths."""
    import numpy as np
    ra, rb = float(prob.inp.ra), float(prob.inp.rb)
    r = ra + np.arange(npts + 1, dtype=np.float64) * ((rb - ra) / float(npts))
    U = prob.wavefunctions(l, 1, n0, count, r=r, deriv=False)[0]
    rtxt = [fortran_g(float(ri), 20, 10) for ri in r]
    paths = []
    for j in range(count):
        paths.append(os.path.join(outdir, "wf_l%d_n%d.dat" % (l, n0 + j)))
        with open(paths[-1], "w") as f:
            for rt_, ui in zip(rtxt, U[j]):
                f.write(rt_ + fortran_g(float(ui), 20, 10) + "\n")
    return paths


def radial_matrix(prob, pairs, g, n0_ini, count_ini, n0_fin, count_fin, deriv=False):
    """D[p, i, f] = <f| g(r) |i> = sum_q w_q g(r_q) u_f(r_q) u_i(r_q), or <f| g(r) d/dr |i> = sum_q w_q g(r_q) u_f(r_q) u_i'(r_q)
    with deriv, for every (l_ini, l_fin) = pairs[p], i < count_ini, f < count_fin (1-based windows from n0_ini, n0_fin): the
    layout of Problem.dipole_matrix.  The sum is the assembly's own Gauss-Legendre quadrature (prob.quadrature()), so g = r,
    g = 1/r and g = 1 with deriv give what dipole_matrix gives with a = (1,0,0), (0,1,0), (0,0,1), up to rounding.  g: a
    callable of the array of points, or an array on the quadrature grid.  NumPy on the host tables of prob.wavefunctions (one
    call per distinct channel and role): for moderate sizes; heavy users call operator_matrix below, which contracts over the
    basis on the GPU (Problem.operator_matrix)."""
    import numpy as np
    r, w = prob.quadrature()
    gw = np.asarray(g(r) if callable(g) else g, dtype=np.float64) * w
    if gw.shape != r.shape:
        raise ValueError("g must give one value per quadrature point (%d), got shape %s" % (r.size, gw.shape))
    pairs = [(int(li), int(lf)) for li, lf in pairs]
    ini, fin = {}, {}
    for li, lf in pairs:
        if li not in ini:
            t = prob.wavefunctions(li, 1, n0_ini, count_ini, deriv=deriv)
            ini[li] = (t[1] if deriv else t)[0]
        if lf not in fin:
            fin[lf] = prob.wavefunctions(lf, 1, n0_fin, count_fin, deriv=False)[0]
    D = np.zeros((len(pairs), count_ini, count_fin))
    for p, (li, lf) in enumerate(pairs):
        D[p] = (ini[li] * gw) @ fin[lf].T
    return D


def operator_matrix(prob, pairs, ops, n0_ini, count_ini, n0_fin, count_fin, a=None):
    """D[p, i, f] = <f| sum_o a[p, o] O_o |i> for every (l_ini, l_fin) = pairs[p], i < count_ini, f < count_fin (1-based windows
    from n0_ini, n0_fin), O_o = g_o(r) or g_o(r) d/dr: ops is a list of (g, deriv), g a callable of the array of points or an array
    on the quadrature grid (prob.quadrature()), as in radial_matrix.  The same quadrature sums as radial_matrix, contracted over
    the basis on the GPU in ONE Problem.operator_matrix call (bspatom_operator_matrix: the band of every operator, A x for all
    initial vectors, the product on the matrix cores).  a: (npairs, nop), or (nop,) for every pair; None requires exactly one
    operator and means coefficient 1."""
    import numpy as np
    ops = list(ops)
    if not ops:
        raise ValueError("ops must name at least one operator")
    r = prob.quadrature()[0]
    G = np.empty((len(ops), r.size))
    deriv = np.zeros(len(ops), dtype=np.int32)
    for o, (g, dv) in enumerate(ops):
        gv = np.asarray(g(r) if callable(g) else g, dtype=np.float64)
        if gv.shape != r.shape:
            raise ValueError("operator %d: g must give one value per quadrature point (%d), got shape %s" % (o, r.size, gv.shape))
        G[o] = gv
        deriv[o] = 1 if dv else 0
    if a is None:
        if len(ops) != 1:
            raise ValueError("a=None needs exactly one operator, got %d" % len(ops))
        a = np.ones(1)
    a = np.asarray(a, dtype=np.float64)
    pairs = [(int(li), int(lf)) for li, lf in pairs]
    if a.shape != (len(ops),) and a.shape != (len(pairs), len(ops)):
        raise ValueError("a must have shape (%d,) or (%d, %d), got %s" % (len(ops), len(pairs), len(ops), a.shape))
    return prob.operator_matrix(pairs, G, deriv, n0_ini, count_ini, n0_fin, count_fin, a)


# ---- response at any complex energy: solves with the banded pencil (Problem.resolvent) -------------------------------------
C_RESPONSE = 137.035999          # the speed of light in atomic units, photoabsorption's


def band_apply(A, X):
    """Y[j] = A x_j for the rows x_j of X (m, n); A (2k-1, n) a full band, A[d + k - 1][i] = A(i, i + d) (the layout of
    Problem.dipole_bands / operator_bands).  X real or complex."""
    import numpy as np
    A, X = np.asarray(A), np.asarray(X)
    k, n = (A.shape[0] + 1) // 2, A.shape[1]
    Y = np.zeros_like(X)
    for d in range(-(k - 1), k):
        lo, hi = max(0, -d), min(n, n - d)                     # rows i with 0 <= i + d < n
        Y[:, lo:hi] += A[d + k - 1, lo:hi] * X[:, lo + d:hi + d]
    return Y


def _absorber_band(prob, absorber):
    """the full band (2k-1, nfun) of W(r) for an absorber given as a callable of the points or an array on the quadrature grid
    (cap_profile), or None"""
    import numpy as np
    if absorber is None:
        return None
    r = prob.quadrature()[0]
    g = np.asarray(absorber(r) if callable(absorber) else absorber, dtype=np.float64)
    if g.shape != r.shape:
        raise ValueError("absorber must give one value per quadrature point (%d), got shape %s" % (r.size, g.shape))
    return prob.operator_bands(g, [0])[0]


def response(prob, l_ini, n_ini, l_fin, a, z, absorber=None, a_left=None):
    """R(z) = (A' c_i)^T (H_{l_fin} - i W - z S)^-1 A c_i for every z of an array (or one z): the second-order response of state
    n_ini (1-based) of channel l_ini through the intermediate channel l_fin, at ANY complex energy -- the sum over every state of
    l_fin without forming one of them (Problem.resolvent: one banded LU per energy).  A = a[0] R_r + a[1] R_{1/r} + a[2] R_{d/dr}
    from dipole_bands, A' likewise from a_left (None: A' = A); c_i from eigvecs; W the band of `absorber` (a callable of the
    points or an array on prob.quadrature()'s grid, e.g. cap_profile; None: no absorber, z must then keep off the box
    eigenvalues).  Both channels must be in the last solve.  Returns complex128 of z's shape."""
    import numpy as np
    RB = prob.dipole_bands()
    ci = prob.eigvecs(l_ini, n_ini, 1)
    comb = lambda co: sum(float(co[o]) * RB[o] for o in range(3))
    b = band_apply(comb(a), ci)
    p = b if a_left is None else band_apply(comb(a_left), ci)
    zz = np.asarray(z, dtype=np.complex128)
    W = _absorber_band(prob, absorber)
    _, R, info = prob.resolvent(l_fin, zz.reshape(-1), b, W=W, P=p, want_x=False)
    if np.any(info != 0):
        raise ArithmeticError("response: z on an eigenvalue of channel %d (%d pivots replaced)" % (l_fin, int(info.max())))
    return R[:, 0, 0].reshape(zz.shape)


def polarizability(prob, n_ini, omega, absorber=None):
    """The dynamic dipole polarizability of the s state n_ini (1-based; channels 0 and 1 in the last solve, made by prob.solve):
    alpha(omega) = [R(E_i + omega) + R(E_i - omega)] / 3 with A = r and l_fin = 1; (2/3) R(E_i) at omega = 0.  Real omega without an
    absorber (below the first excitation: real alpha), or any omega with one.  Returns complex128 of omega's shape."""
    import numpy as np
    om = np.asarray(omega, dtype=np.float64)
    Ei = float(prob.last_E[0 - prob.last_l0, n_ini - 1])
    z = np.stack([Ei + om, Ei - om]).astype(np.complex128)
    R = response(prob, 0, n_ini, 1, (1.0, 0.0, 0.0), z, absorber=absorber)
    return (R[0] + R[1]) / 3.0


def photoabsorption(prob, n_ini, omega, absorber):
    """sigma(omega) = 4 pi omega Im alpha(omega) / c in atomic units (c = 137.035999): with an absorber a smooth function of omega
    across the continuum, no box normalisation, no interpolation over the box states."""
    import numpy as np
    om = np.asarray(omega, dtype=np.float64)
    return 4.0 * np.pi * om * polarizability(prob, n_ini, om, absorber).imag / C_RESPONSE


def response_chain(prob, l_ini, n_ini, path, z, absorber=None, left=None):
    """p^T G_s A_s ... G_2 A_2 G_1 A_1 c_i for every row of z: the response of order nstage + 1 of state n_ini (1-based) of channel
    l_ini, G_j = (H_{l_j} - i W - z_j S)^-1 (Problem.resolvent_chain: every chain on the GPU in one call, no intermediate vector
    on the host).  path: a list of (l, a3), the channel of each resolvent and the dipole_bands coefficients of the operator in
    front of it, A = a3[0] R_r + a3[1] R_{1/r} + a3[2] R_{d/dr}; z: (..., nstage), z[..., j] the energy of resolvent j.  left =
    (l_f, n_f, a3): p = A c_f of a final state (bilinear: for an operator that is not symmetric hand in the coefficients of its
    transpose); None: p = A_1 c_i, as in response.  A_1 c_i and p are formed as response forms them, so one stage is response
    bit for bit.  absorber as in response, on every stage.  Every channel must be in the last solve.  Returns complex128 of
    shape z.shape[:-1]; raises ArithmeticError where response does (a pivot was replaced)."""
    import numpy as np
    path = [(int(l), tuple(float(v) for v in a3)) for l, a3 in path]
    if not path:
        raise ValueError("path must name at least one (l, a3)")
    nstage = len(path)
    zz = np.asarray(z, dtype=np.complex128)
    if zz.ndim < 1 or zz.shape[-1] != nstage:
        raise ValueError("z must have shape (..., %d), got %s" % (nstage, zz.shape))
    RB = prob.dipole_bands()
    ci = prob.eigvecs(l_ini, n_ini, 1)
    comb = lambda co: sum(float(co[o]) * RB[o] for o in range(3))
    b = band_apply(comb(path[0][1]), ci)
    p = b if left is None else band_apply(comb(left[2]), prob.eigvecs(int(left[0]), int(left[1]), 1))
    W = _absorber_band(prob, absorber)
    a = np.array([a3 for _, a3 in path[1:]], dtype=np.float64).reshape(nstage - 1, 3)
    _, R, info = prob.resolvent_chain([l for l, _ in path], zz.reshape(-1, nstage), b, G=RB if nstage > 1 else None,
                                      a=a if nstage > 1 else None, W=W, P=p, want_x=False)
    if np.any(info != 0):
        s = int(np.argmax(info.max(axis=0)))
        raise ArithmeticError("response_chain: z on an eigenvalue of channel %d (%d pivots replaced)" % (path[s][0], int(info.max())))
    return R[:, nstage - 1, 0, 0].reshape(zz.shape[:-1])


def two_photon(prob, n_ini, l_mid, final, omega, absorber=None):
    """The radial two-photon amplitude <f| r G_{l_mid}(E_i + omega) r |i> of the s state n_ini (1-based) to final = (l_f, n_f), for
    every omega of an array (or one): the sum over every state of l_mid (angular factors are the caller's: 1/3 for s - p - s).
    Channels 0, l_mid and l_f in the last solve, made by prob.solve.  Returns complex128 of omega's shape."""
    import numpy as np
    om = np.asarray(omega, dtype=np.float64)
    Ei = float(prob.last_E[0 - prob.last_l0, n_ini - 1])
    r1 = (1.0, 0.0, 0.0)
    return response_chain(prob, 0, n_ini, [(l_mid, r1)], (Ei + om)[..., None], absorber=absorber, left=(final[0], final[1], r1))


def two_photon_ati(prob, n_ini, path2, omega, absorber, left=None):
    """Two photons above threshold: p^T G_{l2}(E_i + 2 omega) r G_{l1}(E_i + omega) r c_i of the s state n_ini with path2 = (l1, l2),
    both resolvents in the continuum -- hence the absorber is not optional -- for every omega of an array.  p = r c_i (left None:
    the diagonal fourth-order response) or r c_f of left = (l_f, n_f).  Returns complex128 of omega's shape."""
    import numpy as np
    om = np.asarray(omega, dtype=np.float64)
    Ei = float(prob.last_E[0 - prob.last_l0, n_ini - 1])
    r1 = (1.0, 0.0, 0.0)
    l1, l2 = path2
    z = np.stack([Ei + om, Ei + 2.0 * om], axis=-1)
    return response_chain(prob, 0, n_ini, [(l1, r1), (l2, r1)], z, absorber=absorber,
                          left=None if left is None else (left[0], left[1], r1))


def cauchy_moments(prob, n_ini, order):
    """The moments (2/3) b^T (G S)^(m-1) G b, m = 1 .. order, of the s state n_ini: b = r c_i, G = (H_1 - E_i S)^-1 -- the oscillator
    strength sums S(-(m+1)) -- from ONE chain of `order` stages with the overlap as the operator in between (R of every stage).
    G(E_i +- omega) = G +- omega G S G + omega^2 G S G S G ..., so alpha(omega) = sum over odd m of moment_m omega^(m-1): m = 1 is
    alpha(0), m = 3 the coefficient of omega^2, and so on.  Hydrogen 1s: 9/2, 43/4, 319/12.  Channels 0 and 1 in the last solve, made
    by prob.solve.  Returns float64 (order,)."""
    import numpy as np
    Ei = float(prob.last_E[0 - prob.last_l0, n_ini - 1])
    b = band_apply(prob.dipole_bands()[0], prob.eigvecs(0, n_ini, 1))
    SBf = prob.operator_bands(np.ones(prob.quadrature()[0].size), [0])
    _, R, info = prob.resolvent_chain(np.ones(order, dtype=np.int32), np.full(order, Ei), b, G=SBf, P=b, want_x=False)
    if np.any(info != 0):
        raise ArithmeticError("cauchy_moments: E_i on an eigenvalue of channel 1 (%d pivots replaced)" % int(info.max()))
    return (2.0 / 3.0) * R[0, :, 0, 0].real


# ---- channels coupled to all orders: one banded LU across the channels (Problem.resolvent_coupled) --------------------------
COUPLED_MAX_BAND = 63                      # BSPATOM_COUPLED_MAX_BAND of include/bspatom.h: resolvent_coupled's half-width limit
COUPLED_WIDE_MAX_BAND = 255                # BSPATOM_COUPLED_WIDE_MAX_BAND: the limit of resolvent_coupled_wide and tdse_spline_wide


def band_transpose(G):
    """The full band(s) of the transposed operator(s): T[..., d + k - 1, i] = G^T(i, i + d) = G[..., -d + k - 1, i + d], zero where
    i + d is outside 0 .. n-1.  An index shuffle, no arithmetic: resolvent_coupled with an entry (cr, cc, 1) on G equals the entry
    (cr, cc, 0) on band_transpose(G) bit for bit."""
    import numpy as np
    G = np.asarray(G)
    k, n = (G.shape[-2] + 1) // 2, G.shape[-1]
    T = np.zeros_like(G)
    for d in range(-(k - 1), k):
        lo, hi = max(0, -d), min(n, n - d)                     # rows i with 0 <= i + d < n
        T[..., d + k - 1, lo:hi] = G[..., -d + k - 1, lo + d:hi + d]
    return T


def _full_to_dense(FB, dtype):
    import numpy as np
    k, n = (FB.shape[0] + 1) // 2, FB.shape[1]
    A = np.zeros((n, n), dtype=dtype)
    for d in range(-(k - 1), k):
        i = np.arange(max(0, -d), min(n, n - d))
        A[i, i + d] = FB[d + k - 1, i]
    return A


def coupled_dense(SB, HB, l, z, couplings, G, a, W=None, w=None, dtype=None):
    """The dense matrix of ONE coupled system in channel-major order (block (c, c') in rows c n .. and columns c' n ..), for small
    checks: diagonal block c = H_l[c] - i W_w[c] - z[c] S, and entry p of `couplings` = (cr, cc, ctr) adds sum_o a[p, o] G[o] (its
    transpose where ctr) to block (cr, cc).  SB (k, n), HB (nl, k, n) upper bands with HB[l] the channel l (Problem.assemble(0, nl));
    G (nop, 2k-1, n) or (2k-1, n); a (ncoup, nop) or (ncoup,) complex; W (nabs, 2k-1, n) or (2k-1, n) full bands, w (nch,) with -1 =
    no absorber, None = W[0] on every channel.  dtype: complex128, or clongdouble for a matrix formed in extended precision."""
    import numpy as np
    dtype = np.complex128 if dtype is None else dtype
    real = np.longdouble if dtype == np.clongdouble else np.float64
    SB, HB = np.asarray(SB), np.asarray(HB)
    k, n = SB.shape
    l = [int(v) for v in np.atleast_1d(l)]
    nch = len(l)
    z = np.broadcast_to(np.asarray(z, dtype=np.complex128), (nch,))
    def sym(UB):                                               # the symmetric matrix of an upper band UB[d, i] = A(i, i + d)
        A = np.zeros((n, n), dtype=real)
        for d in range(k):
            i = np.arange(n - d)
            A[i, i + d] = UB[d, :n - d]
            A[i + d, i] = UB[d, :n - d]
        return A
    M = np.zeros((nch * n, nch * n), dtype=dtype)
    S = sym(SB).astype(dtype)
    if W is not None:
        W = np.asarray(W, dtype=np.float64).reshape(-1, 2 * k - 1, n)
    for c in range(nch):
        D = sym(HB[l[c]]).astype(dtype) - dtype(z[c]) * S
        wc = (0 if W is not None else -1) if w is None else int(np.atleast_1d(w)[c])
        if wc >= 0:
            D = D - dtype(1j) * _full_to_dense(W[wc], real).astype(dtype)
        M[c * n:(c + 1) * n, c * n:(c + 1) * n] = D
    if couplings:
        G = np.asarray(G, dtype=np.float64).reshape(-1, 2 * k - 1, n)
        a = np.asarray(a, dtype=np.complex128).reshape(len(couplings), G.shape[0])
        Gd = [_full_to_dense(g, real).astype(dtype) for g in G]
        for p, (cr, cc, ctr) in enumerate(couplings):
            for o, g in enumerate(Gd):
                M[cr * n:(cr + 1) * n, cc * n:(cc + 1) * n] += dtype(a[p, o]) * (g.T if ctr else g)
    return M


def stark_system(channels, F):
    """The static field F z between `channels` (a list of (l, m)): (couplings, a) for resolvent_coupled with G = dipole_bands()[0],
    the band of r.  For every block of dipole_blocks(channels, kind_pi=1) -- bra position a_ <= ket position b_ -- BOTH directions
    are generated: (a_, b_, 0) and (b_, a_, 1), the second as the transpose, with the same real coefficient F <lf m| cos theta |l0 m>,
    (l+1) / sqrt((2l+1)(2l+3)) between l and l+1 at m = 0.  That is dipole_blocks' angular factor c0 c1 without the reference's phase
    (-1)^(lf + l0), which is -1 on every dipole block (a field of the other direction: the levels do not see it, the vectors do)."""
    import numpy as np
    couplings, a = [], []
    for a_, b_, _l0, _lf, c0, coef in dipole_blocks(channels, kind_pi=1):
        couplings += [(a_, b_, 0), (b_, a_, 1)]
        a += [-float(F) * c0 * coef[0]] * 2
    return couplings, np.asarray(a, dtype=np.complex128)


def floquet_system(channels, nphot, omega, F):
    """A monochromatic field F z cos(omega t) in the Floquet picture: the blocks (channel, n), n = -nphot .. nphot ascending, of the
    parity class that block (channels[0], 0) belongs to (l - l_0 - n even), block c with the energy z - n omega, and the coupling
    (F / 2) z between dipole-coupled channels whose n differ by one.  Returns (blocks, zoff, couplings, a): blocks a list of
    ((l, m), n) -- l of block c is blocks[c][0][0] --, zoff[c] = -n omega to be added to the quasi-energy, couplings and a as
    stark_system returns them (both directions, the second as the transpose)."""
    import numpy as np
    l_0 = channels[0][0]
    blocks = [(ch, nn) for nn in range(-nphot, nphot + 1) for ch in channels if (ch[0] - l_0 - nn) % 2 == 0]
    zoff = np.array([-nn * float(omega) for _, nn in blocks])
    couplings, a = [], []
    for a_, b_, _l0, _lf, c0, coef in dipole_blocks([ch for ch, _ in blocks], kind_pi=1):
        if abs(blocks[a_][1] - blocks[b_][1]) != 1:
            continue
        couplings += [(a_, b_, 0), (b_, a_, 1)]
        a += [-0.5 * float(F) * c0 * coef[0]] * 2             # stark_system's sign
    return blocks, zoff, couplings, np.asarray(a, dtype=np.complex128)


def coupled_eigenpair(prob, l, couplings, G, a, shift, x0, zoff=None, W=None, w=None, iters=3, solver=None):
    """Inverse iteration on the coupled pencil: the eigenvalue lambda next to `shift` of
        (sum_c (H_l[c] - i W_w[c] - (lambda + zoff[c]) S) + V) x = 0,
    every solve one Problem.resolvent_coupled call -- resolvent_coupled_wide where nch k - 1 > 63 -- at z[c] = shift + zoff[c] (a
    dressed energy in a static field: stark_system; a quasi-energy: floquet_system and its zoff).  x0: (nch, nfun), e.g. (c_1s, 0, ..).  Per iteration b = S x (band_apply on every
    channel), y = M(shift)^-1 b, and the Rayleigh quotient of y, lambda = shift + y^T b / y^T S y -- BILINEAR, no conjugate, so it
    is complex when an absorber is present (a width) --, x = y / sqrt(y^T S y).  solver: a callable (l, z, B) -> y (nch, nfun) that
    stands in for the GPU call (a dense solve in the CPU tests); prob then only needs the attribute SB_full, the overlap's full
    band (2k-1, nfun).  Returns (lambda, x, history): history the lambda of every iteration."""
    import numpy as np
    x = np.asarray(x0, dtype=np.complex128)
    nch = x.shape[0]
    SBf = getattr(prob, "SB_full", None)
    if SBf is None:
        SBf = prob.operator_bands(np.ones(prob.quadrature()[0].size), [0])[0]
    zoff = np.zeros(nch) if zoff is None else np.asarray(zoff)
    z = complex(shift) + zoff
    if solver is None:
        # beyond bspatom_resolvent_coupled's half-width (BSPATOM_COUPLED_MAX_BAND) the blocked LU for wide bands answers
        call = prob.resolvent_coupled_wide if nch * prob.k - 1 > COUPLED_MAX_BAND else prob.resolvent_coupled

        def solver(l_, z_, B_):
            X, _, info = call(l_, z_, B_, couplings=couplings, G=G, a=a, W=W, w=w)
            if np.any(info != 0):
                raise ArithmeticError("coupled_eigenpair: the shift is on an eigenvalue (%d pivots replaced)" % int(info.max()))
            return X[0, 0]
    lam, history = complex(shift), []
    for _ in range(iters):
        b = band_apply(SBf, x)
        y = np.asarray(solver(l, z, b), dtype=np.complex128).reshape(nch, -1)
        ysy = np.sum(y * band_apply(SBf, y))
        lam = complex(shift) + np.sum(y * b) / ysy
        x = y / np.sqrt(ysy)
        history.append(lam)
    return lam, x, history


# ---- the TDSE in the spline basis: Crank-Nicolson steps on the coupled LU (Problem.tdse_spline) ------------------------------
def band_symmetric(UB):
    """The full band (2k-1, n) of the symmetric matrix whose upper band is UB (k, n), UB[d, i] = A(i, i + d) (Problem.assemble's SB,
    HB[l]): F[d + k - 1, i] = A(i, i + d), zero where i + d is outside 0 .. n-1.  An index shuffle, no arithmetic: band_apply on it is
    the product b = S c of a Problem.tdse_spline step bit for bit."""
    import numpy as np
    UB = np.asarray(UB)
    k, n = UB.shape
    F = np.zeros((2 * k - 1, n), dtype=UB.dtype)
    for d in range(k):
        F[k - 1 + d, :n - d] = UB[d, :n - d]
        F[k - 1 - d, d:] = UB[d, :n - d]
    return F


def spline_midpoints(t0, dt, nsteps):
    """The times t0 + (n + 1/2) dt, n < nsteps, at which a Crank-Nicolson step of Problem.tdse_spline takes its Hamiltonian"""
    import numpy as np
    return float(t0) + (np.arange(nsteps) + 0.5) * float(dt)


def spline_coefficients(couplings_a, F_mid):
    """The coefficient table of Problem.tdse_spline from a static pattern times the field: couplings_a = (couplings, a) as stark_system
    (with F = 1) returns them -- couplings [(cr, cc, ctr)], a (ncoup,) or (ncoup, nop) --, F_mid the field at the steps' midpoints,
    (nsteps,) for every scan or (nsteps, nscan), real or complex.  Entry p gets a[p] F, a transposed partner (ctr = 1) a[p] conj(F):
    with a partner pattern that is the conjugate of its entry's, the coupling is Hermitian at every step.  Returns complex128
    (nsteps, nscan, ncoup, nop), nscan = 1 for a one-dimensional F_mid (Problem.tdse_spline broadcasts it)."""
    import numpy as np
    couplings, a = couplings_a
    ncoup = len(couplings)
    a = np.asarray(a, dtype=np.complex128).reshape(ncoup, -1)
    F = np.asarray(F_mid, dtype=np.complex128)
    F = F[:, None] if F.ndim == 1 else F
    ctr = np.array([int(t) for _, _, t in couplings], dtype=bool).reshape(ncoup)
    f = np.where(ctr[None, None, :], np.conj(F)[:, :, None], F[:, :, None])          # (nsteps, nscan, ncoup)
    return np.ascontiguousarray(f[..., None] * a[None, None])


def spline_packet(prob, channels, ch, c_vec):
    """A wave packet for Problem.tdse_spline: (nch, nfun) complex, the coefficient vector c_vec (e.g. an eigenvector from eigvecs) in
    position `ch` of `channels`, zero elsewhere"""
    import numpy as np
    c = np.zeros((len(channels), prob.nfun), dtype=np.complex128)
    c[ch] = np.asarray(c_vec).reshape(prob.nfun)
    return c


def spline_propagate(prob, l, c0, dt, nsteps, **kw):
    """Problem.tdse_spline where its LU applies (nch k - 1 <= COUPLED_MAX_BAND) and Problem.tdse_spline_wide beyond it, up to
    COUPLED_WIDE_MAX_BAND: coupled_eigenpair's rule for the two resolvent calls.  The arguments and the results are theirs; where the
    narrow call applies the result has its bits.  ValueError beyond 255."""
    import numpy as np
    nch = np.asarray(l).size
    bw = nch * prob.k - 1
    if bw > COUPLED_WIDE_MAX_BAND:
        raise ValueError("spline_propagate: half-width nch*k - 1 = %d (nch = %d, k = %d) exceeds COUPLED_WIDE_MAX_BAND = %d"
                         % (bw, nch, prob.k, COUPLED_WIDE_MAX_BAND))
    call = prob.tdse_spline_wide if bw > COUPLED_MAX_BAND else prob.tdse_spline
    return call(l, c0, dt, nsteps, **kw)


def split_angular(channels):
    """The angular matrix of the field term for Problem.tdse_split: A[c', c] = <l' m| cos theta |l m> between `channels` (a list of
    (l, m)) -- the factors of stark_system(channels, 1.0), both directions of every dipole block, symmetric, zero elsewhere -- as
    (Q, lam) of numpy.linalg.eigh: A = Q diag(lam) Q^T, Q orthogonal with the eigenvectors in its columns.  The field term of the
    split call is then f(t) A (x) G with G = dipole_bands()[0], what tdse_spline gets from spline_coefficients(stark_system(channels,
    1.0), f)."""
    import numpy as np
    nch = len(channels)
    A = np.zeros((nch, nch))
    couplings, a = stark_system(channels, 1.0)
    for (cr, cc, _t), v in zip(couplings, a):
        A[cr, cc] = v.real
    lam, Q = np.linalg.eigh(A)
    return np.ascontiguousarray(Q), lam


def split_propagate(prob, l, c0, dt, angular, F_mid, G=None, **kw):
    """Problem.tdse_split from the pieces the other helpers give: angular = (Q, lam) of split_angular, F_mid the field at the steps'
    midpoints (spline_midpoints), (nsteps,) for every scan or (nsteps, nscan), real or complex, as spline_coefficients takes it; G
    the radial band, dipole_bands()[0] unless given.  nsteps = len(F_mid).  W, w, P, obs_every, snap_every and the results are
    tdse_split's."""
    import numpy as np
    Q, lam = angular
    F = np.asarray(F_mid, dtype=np.complex128)
    if G is None:
        G = prob.dipole_bands()[0]
    if kw.get("expect") is not None:
        return prob.tdse_split_observe(l, c0, dt, F.shape[0], G=G, Q=Q, lam=lam, f=F, **kw)
    kw.pop("expect", None)
    return prob.tdse_split(l, c0, dt, F.shape[0], G=G, Q=Q, lam=lam, f=F, **kw)


def _split_cos_theta(channels):
    """A[c', c] = <l' m| cos theta |l m> between `channels`: the matrix split_angular diagonalises"""
    import numpy as np
    nch = len(channels)
    A = np.zeros((nch, nch))
    couplings, a = stark_system(channels, 1.0)
    for (cr, cc, _t), v in zip(couplings, a):
        A[cr, cc] = v.real
    return A


def split_expect_dipole(prob, channels):
    """(B, GE) of the induced dipole <z> = <c| cos theta (x) r |c> for Problem.spline_expect and the expect= argument of
    Problem.tdse_split_observe: B (1, nch, nch) the cos theta matrix of stark_system(channels, 1.0) -- split_angular's A, both
    directions of every dipole block, two non-zero entries per row at most --, GE (1, 2k-1, nfun) = dipole_bands()[0], the band of r.
    Both are symmetric: the value is real to rounding."""
    import numpy as np
    return _split_cos_theta(channels)[None], np.ascontiguousarray(prob.dipole_bands()[0][None])


def split_expect_accel(prob, channels, dVdr=None):
    """(B, GE) of the dipole acceleration form <c| cos theta (x) dV/dr |c>, the observable an absorbing boundary does not spoil
    (a(t) = -<dV/dr cos theta> - F(t) for one electron): the B of split_expect_dipole, GE (1, 2k-1, nfun) the operator_bands of dV/dr on
    the quadrature points.  dVdr: the profile on prob.quadrature()[0], or a callable of r; None: zatom / r^2, the Coulomb potential's,
    valid for kind_pot = 0 alone -- with another potential and no profile: ValueError."""
    import numpy as np
    r = prob.quadrature()[0]
    if dVdr is None:
        if int(prob.inp.kind_pot) != 0:
            raise ValueError("split_expect_accel: kind_pot = %d is not the Coulomb potential: give dVdr on the quadrature points"
                             % int(prob.inp.kind_pot))
        g = float(prob.inp.zatom) / (r * r)
    else:
        g = np.asarray(dVdr(r) if callable(dVdr) else dVdr, dtype=np.float64).reshape(r.shape)
    return _split_cos_theta(channels)[None], np.ascontiguousarray(prob.operator_bands(g, [0]))


def split_expect_rows(obs, nch, nproj):
    """The expectation values of the rows of Problem.tdse_split_observe: complex (nobs, nscan, nexp) from obs (nobs, nscan, nch +
    2 nproj + 2 nexp), operator o from the entries nch + 2 nproj + 2 o (Re) and + 1 (Im)."""
    import numpy as np
    obs = np.asarray(obs, dtype=np.float64)
    off = nch + 2 * nproj
    if obs.ndim != 3 or obs.shape[-1] < off or (obs.shape[-1] - off) % 2:
        raise ValueError("split_expect_rows: rows of width %s do not hold nch = %d norms, %d projections and whole complex entries"
                         % (obs.shape[-1:], nch, nproj))
    e = obs[..., off:]
    return e[..., 0::2] + 1j * e[..., 1::2]


def hhg_spectrum(d, dt_rows, window="hann", kind="dipole"):
    """The harmonic spectrum of a dipole or acceleration signal sampled every dt_rows (obs_every * dt): (omega, S), omega = 2 pi
    rfftfreq, S = |omega^2 d~(omega)|^2 for kind = "dipole" (the acceleration's spectrum from the length form) or |a~(omega)|^2 for
    kind = "accel", with x~(omega) = dt_rows sum_n w_n x_n exp(-i omega t_n).  d: (nt,) or (nt, ...), the time on axis 0, real or
    complex (the real part is taken: the observables are real); window "hann" or None.  Pure NumPy."""
    import numpy as np
    x = np.real(np.asarray(d))
    nt = x.shape[0]
    if window == "hann":
        wn = np.hanning(nt)
    elif window is None:
        wn = np.ones(nt)
    else:
        raise ValueError("hhg_spectrum: window %r (\"hann\" or None)" % (window,))
    if kind not in ("dipole", "accel"):
        raise ValueError("hhg_spectrum: kind %r (\"dipole\" or \"accel\")" % (kind,))
    omega = 2.0 * np.pi * np.fft.rfftfreq(nt, float(dt_rows))
    xt = float(dt_rows) * np.fft.rfft(x * wn.reshape((nt,) + (1,) * (x.ndim - 1)), axis=0)
    if kind == "dipole":
        xt = xt * (omega ** 2).reshape((-1,) + (1,) * (x.ndim - 1))
    return omega, np.abs(xt) ** 2


# ---- photoelectron spectra of spline packets: the window operator (Problem.spline_window) -------------------------------------
def _window_integral(m):
    """I_m = integral of 1 / (x^(2m) + 1) over the real line = pi / (m sin(pi / 2m))"""
    import numpy as np
    return np.pi / (m * np.sin(np.pi / (2 * m)))


def window_shifts(E, gamma, m):
    """The shifts of the window operator of order m for Problem.spline_window: z[e, j] = E[e] + gamma exp(i pi (2j + 1) / (2m)),
    j < m, the roots of (lambda - E)^(2m) + gamma^(2m) in the upper half plane (their conjugates are the other m):
    prod_j (lambda - z_j)(lambda - conj z_j) = (lambda - E)^(2m) + gamma^(2m).  E: energies (ne,) or a scalar; returns complex (ne, m)."""
    import numpy as np
    m = int(m)
    if m < 1 or not float(gamma) > 0.0:
        raise ValueError("window_shifts: order m = %r >= 1 and width gamma = %r > 0 are needed" % (m, gamma))
    E = np.atleast_1d(np.asarray(E, dtype=np.float64))
    ph = np.exp(1j * np.pi * (2 * np.arange(m) + 1) / (2 * m))
    return np.ascontiguousarray(E[:, None] + float(gamma) * ph[None, :])


def window_spectrum(prob, l, c, E, gamma, m=2):
    """P_m(E) = <c| gamma^(2m) / ((H_l - E)^(2m) + gamma^(2m)) |c> per scan, channel and energy: (nscan, nch, ne), or (nch, ne) for one
    packet -- the part of every channel's packet within about gamma of E, sum_n |<n|c>|^2 gamma^(2m) / ((E_n - E)^(2m) + gamma^(2m))
    over the box states of that channel, from m banded solves per energy instead of the eigenvectors (Problem.spline_window with
    window_shifts).  The packets must come from a run WITHOUT an absorber on a box that still holds them: the window needs a
    Hermitian H.  Raises RuntimeError if a pivot had to be replaced (it cannot with gamma > 0)."""
    import numpy as np
    N, info = prob.spline_window(l, c, window_shifts(E, gamma, m))
    if np.any(info != 0):
        raise RuntimeError("window_spectrum: replaced pivots at energies %s" % np.flatnonzero(info))
    return float(gamma) ** (2 * int(m)) * N


def window_density(P, gamma, m):
    """dP/dE = P / (gamma I_m), I_m = pi / (m sin(pi / 2m)): a window of order m has the area gamma I_m, so that the integral of the
    density over all energies is the norm c^H S c of the packet (for energy grids finer than gamma)"""
    import numpy as np
    return np.asarray(P, dtype=np.float64) / (float(gamma) * _window_integral(int(m)))


def window_yield(P, E, gamma, m, emin=0.0):
    """The trapezoid integral of window_density(P, gamma, m) over the energies E >= emin, per scan and channel: P (..., ne) on the
    ascending grid E (ne,).  With emin = 0 and a grid that covers the continuum of the box, the ionisation yield per channel."""
    import numpy as np
    E = np.asarray(E, dtype=np.float64).reshape(-1)
    D = window_density(P, gamma, m)
    if D.shape[-1] != E.size or np.any(np.diff(E) <= 0.0):
        raise ValueError("window_yield: P (..., %d) needs an ascending energy grid of that length, got %d" % (D.shape[-1], E.size))
    keep = E >= float(emin)
    if np.count_nonzero(keep) < 2:
        return np.zeros(D.shape[:-1])
    Ek, Dk = E[keep], D[..., keep]
    return np.sum(0.5 * (Dk[..., 1:] + Dk[..., :-1]) * np.diff(Ek), axis=-1)


def spline_yield(obs, nch=None):
    """1 - sum_c N_c of every row of Problem.tdse_spline, (nobs, nscan): with an absorber and a packet normalised to c^H S c = 1, the
    ionisation yield so far.  nch: the channels, when the rows carry projections behind the norms (default: every column is a norm)."""
    import numpy as np
    obs = np.asarray(obs)
    return 1.0 - obs[..., :obs.shape[-1] if nch is None else nch].sum(axis=-1)


# ---- KIND_PI = 0 on several GPUs: one process per GPU, channels sharded, spectra gathered ---------------
def write_structure_outputs(nfun, lmax, E, l_ini, wf, outdir):
    """Enl.dat, wf_n0.dat and the stdout text of a KIND_PI = 0 run from the spectra E[l][i] and the tabulated initial
    state wf = (r, u) (matrices.f90:239-265,388-391; Bsp_Atom.f90:118-146) -- the formatting half of `run`."""
    out = ["PROGRAM TO CALCULATE ELECTRONIC STRUCTURE AND PI CROSS SECTIONS,".rjust(64), "  USING B-SPLINES", ""]
    out.append("Number of B-spline Functions / l: nfun =%5d" % nfun)
    out.append("\nMax. Angular Momenta Included: l_max =%3d" % lmax)
    with open(os.path.join(outdir, "Enl.dat"), "w") as f:
        f.write(" %d\n" % nfun)
        for l in range(lmax + 1):
            out.append("\n l0 = %2d" % l)
            out.append(" HC = ESC eigenvalue solved\n")
            out.append("    n   Eigenvalues")
            out.append("    -   -----------")
            for i in range(nfun):
                txt = fortran_g(E[l][i], 22, 15)
                if i < 20:
                    out.append(" %4d  %s" % (i + 1 + l, txt))
                f.write(" %4d  %s\n" % (i + 1, txt))
            if l == l_ini:
                out.append("\nWriting down Initial State WF\n")
                with open(os.path.join(outdir, "wf_n0.dat"), "w") as g:
                    for ri, ui in zip(*wf):
                        g.write(fortran_g(ri, 20, 10) + fortran_g(ui, 20, 10) + "\n")
    os.makedirs(os.path.join(outdir, "CSs"), exist_ok=True)
    out.append("\nProgram Finished!")
    return "\n".join(out)


def run_sharded(text, outdir=".", npts=10000, solver=None):
    """`Bsp_Atom_omp.x < bsp_0.inp` (KIND_PI = 0) on the GPUs of one node: started once per GPU by
    `python -m torch.distributed.run --nproc-per-node N -m bspatom_amd.host < bsp_0.inp`.  Rank r solves the block of
    l-channels `parallel.channel_range` gives it (the channels are independent, matrices.f90:242-248), the spectra are
    all-gathered (RCCL with backend nccl, gloo without a GPU), the rank that owns l_ini computes the consumed eigenvector
    and its WRITE_WF table and broadcasts them, rank 0 writes the files.  Output identical to `run`.
    solver(l0, nl) -> (E[nl][nfun], wf-or-None) replaces the GPU solve in the CPU tests."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from . import parallel
    if kind_pi_from_namelist(text) != 0:
        raise ValueError("run_sharded covers KIND_PI = 0 (the hot path); the other branches run on one GPU")
    inp = input_from_namelist(text)
    sizes = capi.host_setup(inp, arrays=False)
    nfun, lmax = sizes.nfun, sizes.lmax
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    counts = [parallel.channel_range(r, world, lmax)[1] for r in range(world)]
    l0, nl = parallel.channel_range(rank, world, lmax)
    owner = next(r for r in range(world) if sum(counts[:r]) <= inp.l_ini < sum(counts[:r + 1]))
    use_gpu = solver is None
    dev = torch.device("cuda", torch.cuda.current_device()) if use_gpu else torch.device("cpu")
    wf = None
    if use_gpu:
        prob = capi.Problem(inp, dev.index)
        E_loc = torch.zeros(max(nl, 1) * nfun, dtype=torch.float64, device=dev)
        if nl > 0:
            info = prob.solve_dev(l0, nl, E_loc.data_ptr())
            if info.any():
                raise RuntimeError(" ERROR DIAGONALIZING THE MATRIX! %s (l = %d ..)" % (list(info), l0))
        if rank == owner:
            c = prob.eigvec(inp.l_ini, inp.n0_ini)
            wf = prob.write_wf(c, npts)
        prob.close()
    else:
        E_np, wf = solver(l0, nl)
        E_loc = torch.zeros(max(nl, 1) * nfun, dtype=torch.float64)
        E_loc[: nl * nfun] = torch.from_numpy(np.ascontiguousarray(E_np, dtype=np.float64).reshape(-1))
    E_all = parallel.gather_spectra(E_loc[: nl * nfun], nfun, counts)
    wft = torch.zeros(2 * (npts + 1), dtype=torch.float64, device=dev)
    if rank == owner:
        wft[: npts + 1] = torch.from_numpy(np.asarray(wf[0])).to(dev)
        wft[npts + 1:] = torch.from_numpy(np.asarray(wf[1])).to(dev)
    if world > 1:
        dist.broadcast(wft, src=owner)
    if rank != 0:
        return None
    E = E_all.cpu().numpy()
    w = wft.cpu().numpy()
    return E, write_structure_outputs(nfun, lmax, E, inp.l_ini, (w[: npts + 1], w[npts + 1:]), outdir)


def _main():
    """torchrun entry: namelist on stdin of EVERY rank (torch.distributed.run forwards stdin to rank 0 only, so the text
    can also come from the file named by BSPATOM_INPUT)."""
    import sys
    import torch
    import torch.distributed as dist
    path = os.environ.get("BSPATOM_INPUT")
    text = open(path).read() if path else sys.stdin.read()
    launched = "RANK" in os.environ and "MASTER_ADDR" in os.environ
    # RCCL writes its banner to stdout when the communicator is created: keep the program's stdout clean (it is compared
    # with the reference's), everything else goes to stderr
    real_stdout = os.dup(1)
    sys.stdout.flush()
    os.dup2(2, 1)
    if launched:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            raise SystemExit("bspatom_amd.host needs an MI355X per rank: libbspatom has no CPU path")
    r = run_sharded(text, outdir=os.environ.get("BSPATOM_OUTDIR", "."))
    if r is not None:
        sys.stdout.flush()
        os.write(real_stdout, (r[1] + "\n").encode())
    if launched:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    _main()
