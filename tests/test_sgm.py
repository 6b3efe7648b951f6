"""Dense stereo by semi-global matching (sgm::StereoSGM as PLVS uses it): the oracle's
properties on CPU, and the HIP path against the oracle stage by stage, bit for bit, through the C ABI — on the case
table of tests/sgm_golden_scenario.py also against the digests libsgm's own kernels produced
(tests/golden/sgm_reference_digests.json, tests/test_oracle_pinned_sgm.py)."""
import json
import os

import numpy as np
import pytest

from tests import oracle_lib
from tests import sgm_golden_scenario as S
from tests.oracle_lib import golden

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgm_reference_digests.json")


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def kitti_pair(width=1240, height=376, x0=0, y0=0):
    left, right = golden("urban1_1241x376.pgm"), golden("urban1_right_1241x376.pgm")
    return (np.ascontiguousarray(left[y0:y0 + height, x0:x0 + width]),
            np.ascontiguousarray(right[y0:y0 + height, x0:x0 + width]))


def test_oracle_recovers_a_known_shift(oracle):
    """right = left shifted by 23 px: the disparity is 23 wherever it is defined."""
    img = golden("aloe_640x480.pgm")
    left, right = np.ascontiguousarray(img[:240, :400]), np.ascontiguousarray(img[:240, 23:423])
    disp = oracle.sgm(left, right)
    inner = disp[20:-20, 100:-20]
    assert (inner > 0).mean() > 0.9
    assert (np.abs(inner[inner > 0].astype(int) - 23) <= 1).mean() > 0.98
    # the 16-pixel remainder of check_consistency's grid and the median's border
    assert (disp[0] == 0).all() and (disp[:, 0] == 0).all() and (disp[-1] == 0).all()


def test_oracle_agrees_with_the_sparse_stereo_matcher(oracle):
    """Two independent estimators on a real pair: the dense disparity at an ORB keypoint vs uL - uR of
    Frame::ComputeStereoMatches (oracle/stereo.c)."""
    from tests.test_stereo import KITTI_BF, MB, oracle_side, scale_tables
    left, right = kitti_pair()
    disp, st = oracle.sgm(left, right, stages=True)
    assert (disp > 0).mean() > 0.7
    (kl, dl, pl), (kr, dr, pr) = oracle_side(oracle, left, right, 2000)
    s, inv = scale_tables()
    u, z, score, kept = oracle.stereo_matches(kl, dl, kr, dr, pl, pr, s, inv, MB, np.float32(KITTI_BF))
    ok = (u >= 0) & (kl["octave"] <= 2)
    sparse = kl["x"][ok] - u[ok]
    dense = disp[np.round(kl["y"][ok]).astype(int), np.round(kl["x"][ok]).astype(int)].astype(np.float32)
    both = (dense > 0) & (sparse < 60) & (sparse > 2)
    assert both.sum() > 150
    assert (np.abs(dense[both] - sparse[both]) <= 2.0).mean() > 0.85
    # stage invariants: census is 31 bits and zero on the border; the summed costs of eight paths fit 8 * (P2 + 31)
    assert (st["census_left"] < 2 ** 31).all() and (st["census_left"][:3] == 0).all() and (st["census_left"][:, :4] == 0).all()
    assert st["cost_sum"].max() <= 8 * (120 + 31)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["kitti_1240x376", "odd_333x181", "small_64x48", "flat"])
def test_hip_sgm_matches_oracle(oracle, case):
    from plvs_amd.sgm import StereoSGM
    if case == "kitti_1240x376":
        left, right = kitti_pair()
    elif case == "odd_333x181":
        left, right = kitti_pair(333, 181, 500, 100)
    elif case == "small_64x48":
        left, right = kitti_pair(64, 48, 300, 200)
    else:
        left = np.full((64, 96), 128, np.uint8)
        left[20:40, 30:60] = 0                       # zero pixels are masked by the consistency check
        right = left.copy()
    h, w = left.shape
    want, st = oracle.sgm(left, right, stages=True)
    sgm = StereoSGM(w, h)
    got = sgm.execute(left, right)
    for name in ("census_left", "census_right", "cost_sum", "raw_left", "raw_right", "median_left", "median_right"):
        assert np.array_equal(sgm.stage(name), st[name]), name
    assert np.array_equal(got, want)
    # other parameters, and the device flavour
    import torch
    p = StereoSGM.Parameters(P1=7, P2=60, uniqueness=0.9)
    sgm2 = StereoSGM(w, h, param=p)
    d_out = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    sgm2.execute_dev(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), d_out)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), oracle.sgm(left, right, 7, 60, 0.9))
    with pytest.raises(ValueError):
        StereoSGM(w, h, disparity_size=32)


@pytest.fixture(scope="module")
def reference_digests():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def hip_stages(sgm, final):
    """The stages of the handle's last call, named as S.STAGES (plus cost_sum, which the reference keeps in shared memory)."""
    st = {k: sgm.stage(k) for k in ("census_left", "census_right", "cost_sum", "raw_left", "raw_right", "median_left",
                                    "median_right", "paths")}
    st = S.split_paths(st)
    st["final"] = final
    return st


def assert_stages_equal(got, want):
    for k in S.STAGES + ["cost_sum"]:                    # array for array, so that a mismatch has a location
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if not np.array_equal(got[k], want[k]):
            where = np.argwhere(got[k] != want[k])
            raise AssertionError(f"{k}: {len(where)} of {got[k].size} differ, first at {tuple(where[0])}: "
                                 f"{got[k][tuple(where[0])]} != {want[k][tuple(where[0])]}")


def oracle_stages(oracle, left, right, p1=10, p2=120, u=0.95):
    disp, st = oracle.sgm(left, right, p1, p2, u, stages=True)
    cost_sum = st["cost_sum"]
    st = S.split_paths(st)
    st["cost_sum"], st["final"] = cost_sum, disp
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.CASES, ids=[c["id"] for c in S.CASES])
def test_hip_sgm_equals_oracle_and_reference_digests(oracle, reference_digests, case):
    """Every stage of the HIP path — the eight path volumes one by one — equals the oracle's, and its sha256 the one
    the compiled reference made."""
    from plvs_amd.sgm import StereoSGM
    left, right = S.inputs(case)
    p = StereoSGM.Parameters(P1=case["P1"], P2=case["P2"], uniqueness=case["uniqueness"])
    sgm = StereoSGM(case["width"], case["height"], param=p)
    got = hip_stages(sgm, sgm.execute(left, right))
    sgm.close()
    assert_stages_equal(got, oracle_stages(oracle, left, right, case["P1"], case["P2"], case["uniqueness"]))
    assert S.digests(got) == reference_digests[case["id"]]


@pytest.mark.gpu
def test_create_refuses_a_p2_that_does_not_fit_a_byte():
    """P2 + 31 (the largest matching cost) must fit the byte a path cost is stored in: 224 is the limit, 225 an error."""
    from plvs_amd._lib import PlvsHipError
    from plvs_amd.sgm import StereoSGM
    with pytest.raises(PlvsHipError, match="P2"):
        StereoSGM(65, 33, param=StereoSGM.Parameters(P1=10, P2=225))
    StereoSGM(65, 33, param=StereoSGM.Parameters(P1=224, P2=224)).close()


@pytest.mark.gpu
def test_two_calls_on_one_handle_each_equal_their_own_reference(oracle, reference_digests):
    from plvs_amd.sgm import StereoSGM
    by_id = {c["id"]: c for c in S.CASES}
    sgm = StereoSGM(65, 33)
    for cid in ("noise_65x33", "real_65x33", "zeros_65x33", "stripes_65x33"):     # zeros after real: nothing may be left over
        left, right = S.inputs(by_id[cid])
        got = hip_stages(sgm, sgm.execute(left, right))
        assert_stages_equal(got, oracle_stages(oracle, left, right))
        assert S.digests(got) == reference_digests[cid]


@pytest.mark.gpu
def test_back_to_back_device_calls_on_two_streams(oracle):
    """Two execute_dev calls with different pairs on one handle, on two torch streams, with no host synchronisation
    between them: the handle orders the second after the first (an event recorded at the end of a call, waited on by the
    next call's stream), so the first result is not computed from buffers the second call is already overwriting.
    A passing run cannot prove a race absent — the two calls may simply not have overlapped; the ordering is the code's
    (plvs_hip_sgm_execute_dev), this test holds the results to it."""
    import torch
    from plvs_amd.sgm import StereoSGM
    by_id = {c["id"]: c for c in S.CASES}
    a, b = S.inputs(by_id["real_333x181"]), S.inputs(dict(by_id["swapped_65x33"], width=333, height=181))
    sgm = StereoSGM(333, 181)
    dev = [[torch.from_numpy(x).cuda() for x in pair] for pair in (a, b)]
    outs = [torch.zeros((181, 333), dtype=torch.uint8, device="cuda") for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for (l, r), out, st in zip(dev, outs, streams):
        with torch.cuda.stream(st):
            sgm.execute_dev(l, r, out)
    torch.cuda.synchronize()
    want_a, want_b = oracle_stages(oracle, *a), oracle_stages(oracle, *b)
    assert np.array_equal(outs[0].cpu().numpy(), want_a["final"])
    assert_stages_equal(hip_stages(sgm, outs[1].cpu().numpy()), want_b)
    assert not np.array_equal(want_a["final"], want_b["final"])
