"""Host-only resource-shape planning (kss_plan_shapes): the shape id a staged batch gives every
pod for k_simple's shape table.  Two pods share a shape exactly when the NodeResourcesFit request,
the LeastAllocated (non-zero) request, the BalancedAllocation request and the "every request is
zero" flag of their compact records agree; what only the commit or the static filters read
(AssumePod deltas, PreFilter status, class) is not part of a shape.  Inputs are compiled from
progfuzz manifests (programs=False: a k_simple batch) and then edited field by field, so each
case changes one thing.  Also builds and runs the stand-alone sanitizer check of the host code
(tests/csrc/shape_plan_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import progfuzz
from kss import abi, native
from kss.compile import compile_cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiled(n_pods, requests=None, n_extended=0):
    """n_pods plain pending pods (same requests unless a list is given) on a small cluster."""
    nodes, bound, pods = progfuzz.make(7, 6, n_pods, extended=n_extended > 0, n_extended=max(n_extended, 1),
                                       programs=False)
    for j, p in enumerate(pods):
        p["spec"].pop("initContainers", None)
        req = requests[j] if requests is not None else {"cpu": "250m", "memory": "256Mi"}
        p["spec"]["containers"][0]["resources"]["requests"] = dict(req)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return cc, cp


def _ids(cp, n_scalar=0):
    ids, n = native.plan_shapes(cp.as_struct(), n_scalar)
    return ids.tolist(), n


def test_equal_pods_share_one_shape():
    _, cp = _compiled(5)
    assert _ids(cp) == ([0] * 5, 1)


def test_ephemeral_fit_request_splits():
    _, cp = _compiled(3)
    cp.pods["fit_request"][1][abi.KSS_RES_EPHEMERAL] += 1
    assert _ids(cp) == ([0, 1, 0], 2)


def test_nonzero_request_splits_at_equal_fit_request():
    """The no-request pod: its fit request is zero, its LeastAllocated request the non-zero
    default.  Two such pods that differ in the non-zero request alone are two shapes."""
    _, cp = _compiled(3, requests=[{}, {}, {}])
    assert (cp.pods["fit_request"] == 0).all()
    assert _ids(cp) == ([0, 0, 0], 1)
    cp.pods["score_req_nz"][2][abi.KSS_RES_CPU] += 50
    assert (cp.pods["fit_request"][2] == cp.pods["fit_request"][0]).all()
    assert _ids(cp) == ([0, 0, 1], 2)


def test_balanced_request_splits():
    _, cp = _compiled(2)
    cp.pods["score_req"][1][abi.KSS_RES_MEMORY] += 1
    assert _ids(cp) == ([0, 1], 2)


def test_all_zero_flag_splits():
    """A pod that asks only for an extended resource has the same cpu / memory / ephemeral
    requests as the no-request pod, but fitsRequest does not stop at the pod count for it."""
    cc, cp = _compiled(3, requests=[{}, {}, {}], n_extended=1)
    n_scalar = len(cc.scalars)
    assert n_scalar == 1
    assert _ids(cp, n_scalar) == ([0, 0, 0], 1)
    cp.pods["fit_request"][1][abi.KSS_RES_SCALAR0] = 1
    for f in ("fit_request", "score_req_nz", "score_req"):
        assert (cp.pods[f][1][:3] == cp.pods[f][0][:3]).all()
    assert _ids(cp, n_scalar) == ([0, 1, 0], 2)


def test_commit_status_and_class_are_not_part_of_a_shape():
    _, cp = _compiled(4)
    cp.pods["commit_req"][1][abi.KSS_RES_CPU] += 7
    cp.pods["commit_nz"][1][1] += 7
    cp.pods["prefilter_status"][2] = abi.KSS_PF_NODE_AFFINITY_CONFLICT
    cp.pods["cls"][3] = -1
    cp.pods["priority"][3] = 9
    assert _ids(cp) == ([0] * 4, 1)


def test_ids_follow_first_appearance():
    a, b, c = {"cpu": "100m"}, {"cpu": "200m"}, {"memory": "64Mi"}
    _, cp = _compiled(8, requests=[b, a, b, c, a, c, b, {}])
    assert _ids(cp) == ([0, 1, 0, 2, 1, 2, 0, 3], 4)


@pytest.mark.parametrize("n", [64, 65])
def test_shape_count_at_the_table_limit(n):
    reqs = [{"cpu": "%dm" % (10 * (j % n + 1))} for j in range(2 * n)]
    _, cp = _compiled(2 * n, requests=reqs)
    ids, cnt = _ids(cp)
    assert cnt == n
    assert ids == [j % n for j in range(2 * n)]


def test_empty_podset_has_no_shapes():
    _, cp = _compiled(1)
    s = cp.as_struct()
    s.n_pods = 0
    ids, n = native.plan_shapes(s)
    assert n == 0 and len(ids) == 0


def test_host_shape_code_under_sanitizers(tmp_path):
    """kss_host_assign_shapes / kss_host_shape_key (kss_host.cpp) in a stand-alone program built
    with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "shape_plan_check")
    csrc = os.path.join(ROOT, "kube-scheduler-simulator_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests", "csrc", "shape_plan_check.cpp"), os.path.join(csrc, "kss_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "unsupported" in b.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shape_plan_check ok" in r.stdout
