"""The choice of sampler without a device: the ValueErrors of ``PnpRansac(sample=...)``, ``TrackOdometry(pnp_sample=...)``
and ``device.pnp_ransac_sampled_device``, the argument walk of the new entry, and the plan through host/build/pnp_plan_cli with the
sampler argument: sample size 4, no LDS for the hypotheses, the bytes of "dlt6", and the refusal of an unknown sampler."""
import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

K = (512.0, 512.0, 319.5, 239.5)


def _call(w, n=40, sample="p3p", hyp=True):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    return D.pnp_ransac_sampled_device(w.ctx, w.t("landmarks", "float32", n, 3), w.t("uv", "float32", n, 2), w.t("status", "uint8", n), K, 1.0, 64, 4, 0, sample,
                                       w.t("workspace", "int64", -(-N.pnp_ransac_workspace_bytes(n, 64, 4) // 8)), w.t("pose", "float32", 7),
                                       w.t("n_inliers", "int32", 1), w.t("best", "int32", 1), w.t("valid", "int32", 1),
                                       w.t("counts", "int32", 64) if hyp else None, w.t("models", "float32", 64, 12) if hyp else None)


def test_the_sampled_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    A.walk_call(monkeypatch, _call, ["ftk_pnp_ransac_sampled_device"])
    A.walk_call(monkeypatch, lambda w: _call(w, hyp=False), ["ftk_pnp_ransac_sampled_device"])


@pytest.mark.parametrize("bad", ["P3P", "epnp", "", None, 1, b"p3p"])
def test_a_bad_sampler_is_a_value_error_before_a_device_is_touched(monkeypatch, bad):
    import feature_tracker_amd as F
    w = A.Walk(monkeypatch)
    with pytest.raises(ValueError, match="sample"):
        F.PnpRansac(K, sample=bad)
    with pytest.raises(ValueError, match="pnp_sample"):
        F.TrackOdometry(K, pnp_sample=bad)
    with pytest.raises(ValueError, match="sample"):
        _call(w, sample=bad)
    assert w.lib.calls == []


def test_both_names_are_taken():
    import feature_tracker_amd as F
    assert F.PnpRansac(K).sample == "dlt6" and F.PnpRansac(K, sample="p3p").sample == "p3p"
    assert F.TrackOdometry(K).pnp_sample == "dlt6" and F.TrackOdometry(K, pnp_sample="p3p")._pnp.sample == "p3p"


def test_the_plan_with_the_sampler_argument():
    from feature_tracker_amd import _native as N
    shapes = [(n, k, r) for n in (1, 4, 257, 65536) for k in (1, 64, 65, 4096) for r in (0, 4)]
    plain = A.run_plan_tool(A.plan_cli("pnp_plan_cli"), shapes)
    dlt6 = A.run_plan_tool(A.plan_cli("pnp_plan_cli"), [s + (N.FTK_PNP_SAMPLE_DLT6,) for s in shapes])
    p3p = A.run_plan_tool(A.plan_cli("pnp_plan_cli"), [s + (N.FTK_PNP_SAMPLE_P3P,) for s in shapes])
    for (n, k, r), a, b, c in zip(shapes, plain, dlt6, p3p):
        assert "sample" not in a and all(b[key] == v for key, v in a.items())  # the old argument list prints what it printed
        assert (int(b["sampler"]), int(b["sample"])) == (0, N.FTK_PNP_SAMPLE) and int(b["hyp_lds"]) == 4 * 156 * 64
        assert (int(c["sampler"]), int(c["sample"])) == (1, 4) and N.FTK_PNP_P3P_SAMPLE == 4 and int(c["hyp_lds"]) == 0
        assert int(c["bytes"]) == int(a["bytes"]) == N.pnp_ransac_workspace_bytes(n, k, r) and int(c["launches"]) == 5 + 2 * r
        assert {key: v for key, v in c.items() if key not in ("sampler", "sample", "hyp_lds")} == {key: v for key, v in a.items() if key != "hyp_lds"}
    refused = A.run_plan_tool(A.plan_cli("pnp_plan_cli"), [(8, 64, 4, 2), (8, 64, 4, -1), (0, 64, 4, 1)])
    assert [p["refused"] for p in refused] == ["sampler", "sampler", "sizes"]


def test_nothing_in_the_package_imports_the_restatements():
    A.nothing_in_the_package_imports("pnp_p3p_ref")
    A.nothing_in_the_package_imports("pnp_p3p_ref64")
