"""hdn_amd.simi_training_forward on the device against the float64 CPU twin of tests/simi_train_cases.py: the fourteen outputs and every parameter
gradient within the chain bound max(4 d_ref, 1e-5); a batch with no unsupervised positive (sim_loss, cor_err_sim and their gradients exactly zero,
total_loss finite); HomoModelBuilder.training_forward(host_free=True) against host_free=False; forward + backward captured in one graph and replayed
after the inputs and flags are refilled in place.  The host part (no `gpu` mark) holds the twin's argmax margins against the fp32 twin's error."""
import pytest
import torch

import simi_train_cases as ST
from hdn_amd import SimiTrainConfig, simi_training_forward  # noqa: F401  (the module is about them: without them nothing here is collected)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    """The stand-in on the device.  Its small convolutions are the library's, which picks an algorithm per process: pinned for this module's tests,
    as tests/test_gpu_triplet.py pins its end-to-end step."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield ST.on_device(ST.make_model(), dev)
    torch.backends.cudnn.deterministic = prev


def _to(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


def _run(model, data):
    """(outputs, counts, parameter gradients of total_loss) of one eager call"""
    import hdn_amd
    model.zero_grad(set_to_none=True)
    out, counts = hdn_amd.simi_training_forward(model, data, return_counts=True)
    out["total_loss"].backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    return {k: v.detach().clone() for k, v in out.items()}, counts, grads


# ------------------------------------------------------------------------------------------------------------------------------------- host part
def test_the_twin_has_argmax_margins_no_rounding_can_cross():
    """On the CPU: in the float64 twin the best class-1 logit (:377) and the best logit difference (:390: the softmax probability is monotone in it)
    lead the runner-up by far more than the fp32 twin deviates from float64, and both twins pick the cells of the priors."""
    for flags in ("mixed",):
        t = ST.twin(flags)
        m64, m32 = t[torch.float64][2], t[torch.float32][2]
        for key, cells, S, score in (("cls", ST.CELLS, 25, lambda c: c[:, 1]), ("cls_lp", ST.CELLS_LP, 13, lambda c: c[:, 1] - c[:, 0])):
            s64 = score(m64[key]).reshape(ST.B, -1)
            top = torch.topk(s64, 2, dim=1).values
            lead = float((top[:, 0] - top[:, 1]).min())
            err = ST.deviation(score(m32[key]), score(m64[key]))
            print(f"SIMI_TRAIN margin {key}: lead {lead:.3f}, fp32 twin error {err:.3g}")
            assert lead > 1.0 and lead > 1000 * err
            want = torch.tensor([r * S + c for r, c in cells])
            which = "best" if key == "cls" else "best_lp"
            assert torch.equal(m64[which], want) and torch.equal(m32[which], want)
        assert [int(v) for v in m64["counts"]] == [3, 2, 1, 2, 1, 2]              # n_sup, n_sup_pos, n_sup_neg, n_unsup, n_unsup_pos, n_neg
        out64 = t[torch.float64][0]
        assert all(bool(torch.isfinite(v)) for v in out64.values())
        assert all(float(out64[k]) > 0 for k in ("sim_loss", "homo_unsup_loss", "cor_err", "cor_neg_loss", "sim_cent_loss", "total_loss"))


def test_the_configuration_and_the_model_are_checked_before_any_device_work():
    import hdn_amd
    from hdn_amd import _lib
    from hdn_amd.simi_train import DATA_KEYS
    cfg = hdn_amd.SimiTrainConfig()
    assert (cfg.stride, cfg.stride_lp, cfg.exemplar_size, cfg.instance_size, cfg.output_size_lp) == (8, 8, 127, 255, 13)
    assert (cfg.cls_weight, cfg.loc_weight, cfg.obj, cfg.model_type, cfg.weighted_map_lp, cfg.adjust) == (1.0, 1.0, "ALL", "E2E", False, True)
    assert set(DATA_KEYS) == set(ST.make_batch())
    model, batch = ST.make_model(), ST.make_batch()
    for bad in (dict(obj="HOMO"), dict(model_type="SEP"), dict(weighted_map_lp=True), dict(stride=16), dict(stride_lp=4), dict(exemplar_size=128),
                dict(instance_size=256), dict(output_size_lp=15), dict(cls_weight="1"), dict(adjust=1)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            hdn_amd.simi_training_forward(model, batch, hdn_amd.SimiTrainConfig(**bad))
    hdn_amd.SimiTrainConfig(cls_weight=2.0, loc_weight=1.2, adjust=False).validate()
    with pytest.raises(TypeError):
        hdn_amd.simi_training_forward(model, batch, {"stride": 8})
    with pytest.raises(KeyError, match="search_poly"):
        hdn_amd.simi_training_forward(model, {k: v for k, v in batch.items() if k != "search_poly"})
    with pytest.raises(_lib.HdnHipError):                                        # the batch is on the host: nothing is uploaded, no fallback
        hdn_amd.simi_training_forward(model, batch)
    import copy
    broken = copy.deepcopy(model)
    broken.neck_lp = None
    with pytest.raises(AttributeError, match="neck_lp"):
        hdn_amd.simi_training_forward(broken, batch)
    broken = copy.deepcopy(model)
    broken.hm_net.ShareFeature.hip_train = False                                 # eval() without hip_train detaches
    with pytest.raises(RuntimeError, match="ShareFeature.*eval.*hip_train"):
        hdn_amd.simi_training_forward(broken, batch)
    assert hdn_amd.simi_training_forward is hdn_amd.simi_train.simi_training_forward


# -------------------------------------------------------------------------------------------------------------------------------------- GPU part
@gpu
def test_outputs_and_parameter_gradients_against_the_float64_twin(dev, model):
    import hdn_amd
    t = ST.twin("mixed")
    (out64, g64, mid64), (out32, g32, _) = t[torch.float64], t[torch.float32]
    out, counts, grads = _run(model, _to(ST.make_batch("mixed"), dev))
    assert tuple(out) == hdn_amd.corner.OUTPUT_KEYS == ST.OUTPUT_KEYS
    assert counts["corner"].cpu().tolist() == [int(v) for v in mid64["counts"]] and counts["sim"].cpu().tolist() == [1, 2]
    failed = []
    for k in ST.OUTPUT_KEYS:
        d, d_ref = ST.deviation(out[k].cpu(), out64[k]), ST.deviation(out32[k], out64[k])
        print(f"SIMI_TRAIN {k}: value {float(out[k]):.9g} float64 {float(out64[k]):.9g} d {d:.3g} d_ref {d_ref:.3g} bound {ST.bound(d_ref):.3g}")
        if not d <= ST.bound(d_ref):
            failed.append(k)
    assert set(grads) == set(g64)
    for k in sorted(g64):
        assert (grads[k] is None) == (g64[k] is None), k
        if g64[k] is None:
            continue
        d, d_ref = ST.deviation(grads[k].cpu(), g64[k]), ST.deviation(g32[k], g64[k])
        print(f"SIMI_TRAIN grad {k}: max |g64| {float(g64[k].abs().max()):.3g} d {d:.3g} d_ref {d_ref:.3g} bound {ST.bound(d_ref):.3g}")
        if not d <= ST.bound(d_ref):
            failed.append("grad " + k)
    assert not failed, failed
    assert sum(v is not None and bool((v != 0).any()) for v in g64.values()) >= 20          # the loss reaches every network of the model


@gpu
def test_no_unsupervised_positive_gives_exact_zeros_and_a_finite_total(dev, model):
    import hdn_amd
    data = _to(ST.make_batch("no_unsup_pos"), dev)
    model.zero_grad(set_to_none=True)
    out, counts = hdn_amd.simi_training_forward(model, data, return_counts=True)
    assert counts["sim"].cpu().tolist() == [0, 2] and counts["corner"].cpu().tolist()[3:5] == [1, 0]
    val = {k: float(v.detach()) for k, v in out.items()}
    assert val["sim_loss"] == 0.0 and val["cor_err_sim"] == 0.0
    assert val["homo_unsup_loss"] == 0.0                                         # n_unsup = 1, nobody selected: 0, where the reference divides by zero
    assert val["total_loss"] == val["total_loss"] and 0 < val["total_loss"] < float("inf")
    params = [p for p in model.parameters()]
    for key in ("sim_loss", "cor_err_sim"):
        gr = torch.autograd.grad(out[key], params, retain_graph=True, allow_unused=True)
        assert all(g is None or not bool((g != 0).any()) for g in gr), key
    out["total_loss"].backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in params)


@gpu
def test_host_free_homography_forward_agrees_with_the_default_path(dev, model):
    """feature_loss and homo_neg_loss of training_forward(host_free=True) against host_free=False on the same data, for a batch with a negative and
    for one without (where every sample is summed and n_sel divides).  The bound is the chain bound of homo_unsup_loss, the same quantity."""
    from hdn_amd.simi_train import homo_constants
    t = ST.twin("mixed")
    d_ref = ST.deviation(t[torch.float32][0]["homo_unsup_loss"], t[torch.float64][0]["homo_unsup_loss"])
    hm = model.hm_net
    for flags in ("mixed", "no_neg"):
        b = _to(ST.make_batch(flags), dev)
        org = torch.cat([b["template_hm"].mean(1, keepdim=True), b["search_hm"][:, :, 64:191, 64:191].mean(1, keepdim=True)], 1).contiguous()
        h4p, patch_indices = homo_constants(ST.B, dev)
        data = {"org_imgs": org, "input_tensors": org, "h4p": h4p, "patch_indices": patch_indices, "if_pos": b["if_pos"], "if_unsup": b["if_unsup"]}
        res = {}
        for host_free in (False, True):
            hm.zero_grad(set_to_none=True)
            out = hm.training_forward(data, host_free=host_free)
            (out["feature_loss"].sum() + out["homo_neg_loss"]).backward()
            res[host_free] = (out, {k: p.grad.detach().clone() for k, p in hm.named_parameters() if p.grad is not None})
        assert set(res[True][0]) == set(res[False][0])                           # the same keys
        for k in ("feature_loss", "homo_neg_loss"):
            a, c = res[True][0][k].detach(), res[False][0][k].detach()
            assert a.shape == c.shape
            d = ST.deviation(a.cpu(), c.cpu())
            print(f"SIMI_TRAIN host_free {flags} {k}: {a.flatten().tolist()} against {c.flatten().tolist()}, d {d:.3g} bound {ST.bound(d_ref):.3g}")
            assert d <= ST.bound(d_ref), (flags, k)
            if flags == "no_neg" and k == "homo_neg_loss":
                assert float(a) == 0.0 == float(c)
            else:
                assert float(a.sum()) > 0, (flags, k)
        assert set(res[True][1]) == set(res[False][1])
        for k, g in res[True][1].items():
            assert ST.deviation(g.cpu(), res[False][1][k].cpu()) <= ST.bound(d_ref), (flags, k)


@gpu
def test_forward_and_backward_in_one_graph_follow_inputs_and_flags_refilled_in_place(dev, model):
    """Warm-up on a side stream, one capture of simi_training_forward and total_loss.backward() under the capture error mode "global" (a stray host
    read or upload fails the capture), then the inputs and the flags are refilled in place and the graph is replayed: the losses are bit-equal to an
    eager call, the parameter gradients within the chain bound (no image requires grad, so no atomic sum is involved)."""
    import hdn_amd
    t = ST.twin("mixed")
    g_ref = {k: ST.deviation(t[torch.float32][1][k], v) for k, v in t[torch.float64][1].items() if v is not None}
    static = {k: v.clone() for k, v in _to(ST.make_batch("mixed"), dev).items()}
    params = dict(model.named_parameters())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                                       # the constants of this batch size are built here, outside the capture
            model.zero_grad(set_to_none=True)
            hdn_amd.simi_training_forward(model, static)["total_loss"].backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="global"):
        out = hdn_amd.simi_training_forward(model, static)
        out["total_loss"].backward()
    captured = {k: p.grad for k, p in params.items() if p.grad is not None}
    assert len(captured) == len(g_ref)
    seen = set()
    for flags, seed in (("no_unsup_pos", 1), ("mixed", 0), ("no_neg", 2), ("mixed", 0)):
        for k, v in _to(ST.make_batch(flags, seed), dev).items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.detach().clone() for k, v in out.items()}
        got_g = {k: v.detach().clone() for k, v in captured.items()}
        eager, _, eager_g = _run(model, static)
        torch.cuda.synchronize()
        for k in ST.OUTPUT_KEYS:
            assert torch.equal(got[k].view(torch.int32), eager[k].view(torch.int32)), (flags, k, float(got[k]), float(eager[k]))
        for k, v in got_g.items():
            assert ST.deviation(v.cpu(), eager_g[k].cpu()) <= ST.bound(g_ref[k]), (flags, k)
        seen.add((float(got["sim_loss"]) > 0, float(got["cor_neg_loss"]) > 0))
        for k, p in params.items():                                              # the eager call replaced .grad: hand the captured buffers back
            p.grad = captured.get(k)
    assert len(seen) >= 2                                                        # the sets were emptied and refilled
    out64 = t[torch.float64][0]                                                  # the last replay is the twin's batch
    for k in ST.OUTPUT_KEYS:
        d_ref = ST.deviation(t[torch.float32][0][k], out64[k])
        assert ST.deviation(got[k].cpu(), out64[k]) <= ST.bound(d_ref), k
