"""The compiled kernels against the reference's own outputs at mid and long
reads (tests/golden/nw_pairs_mid_long, the mid- and long-read e2e cases): the
fixtures, not the oracle, are the judge here.  Which kernel a launch ran is
read from its diagnostics line (IMSAME_NW_PROF) and from the call's launch
masks, so a route that quietly took another kernel fails.

The e2e cases also run through every test parametrised over G.e2e_cases()
(tests/test_gpu.py: oracle parity, the CLI's bytes, slices, devices)."""
import collections
import hashlib

import numpy as np
import pytest

from imsame_amd import Device, render, fasta, FLAG_NW32, FLAG_NW16
from tests import golden_io as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


def _expected_kernel(route, cls, ig, eg, rows):
    """prefixes of the kernel-table row (imsame_dev.hip:NW_KERNELS) the launch must name"""
    if route == "nw32" or ig > 0 or eg > 0:
        return ("nw_kernel<",)                          # int32: forced, or a positive gap term
    if cls == "short":
        return ("nw16_kernel<",) if G.mid_form_fits(ig, eg, rows) else ("nw_kernel<",)
    if cls == "mid" and G.mid_form_fits(ig, eg, rows):
        return ("nw16_mid_kernel<",)
    return ("nwl_kernel",) if route == "nwl" else ("nwp_kernel", "nwl_kernel")


@pytest.mark.parametrize("route", ["auto", "nw32", "nwl"])
def test_nw_pairs_mid_long_match_reference_golden(dev, route, monkeypatch, capfd):
    """Device.nw_pairs over the mid/long NW fixture, one launch per gap pair
    and class of read length (<= 160, 161 .. 320, longer): every field and the
    sha1 of the text rendered from the device's path equal the reference's.
    auto: rows of 161 .. 320 columns run the packed kernel's mid form wherever
    its range proof admits the launch's gaps and longest record, longer ones
    the long-read kernels; nw32: the int32 kernel for every row; nwl: the
    int32 long-read kernel (IMSAME_NWP=0) for what the long-read kernels
    take.  The rows per kernel are printed and must not be zero."""
    monkeypatch.setenv("IMSAME_NW_PROF", "1")
    if route == "nwl":
        monkeypatch.setenv("IMSAME_NWP", "0")
    ran, n_text, n_rows = collections.Counter(), 0, 0
    for cls in G.NW_CLASSES:
        for (ig, eg), rs in G.nw_mid_long_groups(cls).items():
            want = _expected_kernel(route, cls, ig, eg, rs)
            if route == "nwl" and want != ("nwl_kernel",):
                continue
            X, Y = [r["X"].encode() for r in rs], [r["Y"].encode() for r in rs]
            p = dev.params(igap=ig, egap=eg, min_coverage=1e-9, min_identity=1e-9,
                           flags=FLAG_NW32 if route == "nw32" else 0)
            capfd.readouterr()
            res, paths, _ = dev.nw_pairs(X, Y, p, want_paths=True)
            err = capfd.readouterr().err
            names = [ln.split(None, 1)[1] for ln in err.splitlines() if ln.startswith("[nw-kernel] ")]
            assert len(names) == 1 and names[0].startswith(want), (cls, ig, eg, names, want)
            ran[names[0].split("<")[0], cls] += len(rs)
            n_rows += len(rs)
            for k, r in enumerate(rs):
                for f in G.NW_FIELDS:
                    assert int(res[k][f]) == r[f], (route, f, ig, eg, len(r["X"]), len(r["Y"]), r["kind"])
                if res[k]["status"] == 1:
                    txt, ident = render(X[k], Y[k], res[k],
                                        paths[res[k]["path_off"]:res[k]["path_off"] + res[k]["path_len"]])
                    assert len(txt) == r["text_len"] and hashlib.sha1(txt).hexdigest() == r["text_sha1"], (route, ig, eg, k)
                    assert ident == r["identities"]
                    n_text += 1
    print(f"nw_pairs_mid_long [{route}]: rows per kernel and class {dict(ran)}, texts {n_text} of {n_rows}")
    if route == "auto":
        assert n_rows >= 280 and n_text >= 250
        assert ran["nw16_mid_kernel", "mid"] >= 60
        assert ran["nwp_kernel", "long"] + ran["nwl_kernel", "long"] >= 80
        assert not [k for k in ran if k[0] == "nw16_mid_kernel" and k[1] != "mid"]
    elif route == "nw32":
        assert n_rows >= 280 and set(k[0] for k in ran) == {"nw_kernel"}
    else:
        assert ran["nwl_kernel", "long"] >= 80 and ran["nwl_kernel", "mid"] > 0


@pytest.mark.parametrize("name", G.MID_LONG_E2E)
def test_align_matches_reference_golden_headers(dev, name):
    """Device.align on the mid- and long-read e2e cases at every recorded
    -n_threads, default route and packed kernel forced: the accepted reads,
    their records, identity, coverage and length are what the reference wrote
    into its .align headers.  The launch masks prove the class of kernel:
    reads of 161 .. 320 bases stay on the packed kernel (mid_reads: every
    launch, none on the long-read kernel, with allow_too_long and at these
    small launch sizes too), reads above 320 take the long-read kernel."""
    case = G.e2e_case(name)
    db, dbs, brk = fasta.load(case["db"], True)
    q, qs, _ = fasta.load(case["query"])
    lens = np.diff(np.concatenate([qs, [len(q)]]).astype(np.int64))
    dev.index(db, dbs, brk)
    dev.set_query(q, qs)
    for T, run in case["meta"]["runs"].items():
        want = G.headers_of(run["headers"])
        for flags in (0, FLAG_NW16):
            p = G.case_params(dev.params, case)
            p.flags = flags
            res, _, st = dev.align(n_threads=int(T), params=p, allow_too_long=True)
            assert G.result_headers(res) == want, (name, T, flags)
            every = (1 << min(int(st.nw_launches), 64)) - 1
            assert st.nw_launches > 0
            if name == "mid_reads":
                assert lens.min() > 160 and lens.max() <= 320
                assert st.launch_pk == every and st.launch_nwp == 0, (T, flags, st.launch_pk, st.launch_nwp)
            if name == "mid_mixed":
                assert st.launch_pk != 0 and st.launch_nwp != 0 and (st.launch_pk & st.launch_nwp) == 0
            if name == "long_reads":
                assert lens.min() > 320 and st.launch_nwp == every and st.launch_pk == 0
