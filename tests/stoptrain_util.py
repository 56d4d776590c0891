"""What the GPU tests of stop-net training share (tests/test_gpu_stoptrain.py, tests/test_gpu_stoptrain_shapes.py): the cases trained on
the device, one launch per case, and the comparisons with the restatement of tests/stoptrain_ref.py.  Nothing here is derived from what
the GPU returns: the allowance is the case's own (stoptrain_ref.case_reference)."""
import numpy as np

from tests import stoptrain_ref as R

INT_FIELDS = ("n_epochs", "best_epoch", "status", "val_correct", "n_dead_units")


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def trained_cases(names):
    """a module fixture's body -- per case: the restatement's answers (computed once, left unchanged) and the device's, from ONE launch
    of all of its runs; the trainers are closed behind the yield"""
    from dsp_amd import consumers as dc
    out = {}
    for name in names:
        c = dict(R.case_reference(name))
        t = dc.StopTrainer(c["n_coef"], c["max_frames"], c["units"])
        c["d_mfcc"] = cuda(c["mfcc"])
        c["got_mean"], c["got_scale"] = t.set(c["d_mfcc"], c["frame_offsets"], scaler_rows=c["train_rows"])
        res, hist, prob, params = t.train(c["runs"], c["labels"])
        c["trainer"], c["res"], c["hist"], c["prob"], c["params"] = t, res, hist.cpu().numpy(), prob.cpu().numpy(), params.cpu().numpy()
        out[name] = c
    yield out
    for c in out.values():
        c["trainer"].close()


def check_scaler_and_rows(c):
    """the fitted Scaler equals the restatement's float64 results rounded to float32 bit for bit (the restatement takes the kernel's
    summation tree), in the layout dsp_stop_model_params reads; Z equals the inference expression bit for bit -> Z"""
    assert np.array_equal(c["got_mean"], c["mean"]) and np.array_equal(c["got_scale"], c["scale"])
    z = c["trainer"].rows()
    assert z.shape == c["z"].shape == (c["labels"].size, c["trainer"].f_used) and np.array_equal(z.view(np.uint32), c["z"].view(np.uint32))
    net_div = np.where(c["scale"] == 0, np.float32(1), c["scale"])
    idx = R.used_index(c["n_coef"], c["max_frames"], z.shape[1] // c["n_coef"])
    x = R.features(c["mfcc"], c["frame_offsets"], c["n_coef"], c["max_frames"])
    assert np.array_equal(z, ((x - c["mean"][idx]).astype(np.float32) / net_div[idx]).astype(np.float32))   # consumer_ref.StopNet.standardise
    return z


def run_differences(c, k):
    """the worst relative differences of run k's history, params and prob from the restatement's"""
    run, ref = c["runs"][k], c["numpy"][k]
    hist = np.full((max(r["epochs"] for r in c["runs"]), 2), np.nan)
    hist[:run["epochs"]] = ref["history"]
    return {"history": R.relative(c["hist"][k], hist), "params": R.relative(c["params"][k], ref["params"]), "prob": R.relative(c["prob"][k], ref["prob"])}


def check_trajectories(c):
    """history, params and prob within the imported allowance, the integer results exactly -- after asserting that the restatement's
    deciding comparisons have their margin"""
    for k, ref in enumerate(c["numpy"]):
        assert ref["margin"] > 1e-6 and ref["p_margin"] > 1e-6
        got = c["res"][k]
        worst = run_differences(c, k)
        print(f"{c['name']} run {k}: {worst}, allowance {c['allow']:.1e}")
        for field in INT_FIELDS:
            assert got[field] == ref[field], (k, field, got[field], ref[field])
        assert max(worst.values()) <= c["allow"], (k, worst)
        assert abs(got["best_val_loss"] - ref["best_val_loss"]) <= c["allow"] * abs(ref["best_val_loss"])
        assert abs(got["last_loss"] - ref["last_loss"]) <= c["allow"] * abs(ref["last_loss"])


def result_bytes(res, hist, prob, params, k):
    return res[k].tobytes(), hist[k].cpu().numpy().tobytes(), prob[k].cpu().numpy().tobytes(), params[k].cpu().numpy().tobytes()


def check_round_trip(c, k, rows):
    """run k's fitted model through dsp_stop_model_from_training -> dsp_stop_model_create -> dsp_stop_predict_device on the dataset's own
    MFCC reproduces d_prob on `rows` within StopNet's own first-order bound (the one tests/test_gpu_consumer_models.py uses)"""
    import dsp_amd
    from dsp_amd import consumers as dc
    from tests import consumer_ref as CR
    model = dc.stop_model_from_training(c["n_coef"], c["max_frames"], c["units"], c["params"][k], c["got_mean"], c["got_scale"])
    want = R.model_from_training(c["n_coef"], c["max_frames"], c["units"], c["params"][k], c["mean"], c["scale"])
    for key in want:
        assert np.array_equal(np.asarray(model[key]), np.asarray(want[key])), key
    sm = dsp_amd.StopModel(model)
    fo = c["frame_offsets"]
    frames = np.diff(fo)
    if (frames == frames[0]).all():
        got = sm.predict(c["d_mfcc"].reshape(frames.size, int(frames[0]), c["n_coef"])).cpu().numpy()
    else:                                                                                        # a ragged set: a clip a call
        got = {i: float(sm.predict(c["d_mfcc"][fo[i]:fo[i + 1]].reshape(1, -1, c["n_coef"])).cpu().numpy()[0]) for i in rows}
    net = CR.StopNet(model)
    for i in rows:
        p, bound = net.prob(c["mfcc"][fo[i]:fo[i + 1]])
        # the float32 net against its own reference, and against the float64 training-time probability: the parameters' float32
        # rounding (2^-24 relative per layer-1 term, inside the bound's 2^-22) and the float32 tail (a few 1e-7)
        assert abs(float(got[i]) - float(p)) <= bound + 1e-6
        assert abs(float(got[i]) - c["prob"][k][i]) <= 2 * bound + 2e-6, (i, got[i], c["prob"][k][i], bound)
    sm.close()
