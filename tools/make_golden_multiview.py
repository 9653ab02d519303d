#!/usr/bin/env python3
"""Generate tests/golden/golden_multiview_cars3.npz: a three-view object optimised with the UNMODIFIED reference's own terms.

Runs only where the reference tree exists (oracle/ref_shim.py).  The reference optimises an object from one observation; this tool calls
its compute_sdf_loss, compute_render_loss, compute_rotation_loss_sim3, get_robust_res and exp_sim3 once per view at T_oc_v = T_oc @ T_ref_v
and pools the rows with the loop below, which repeats reconstruct/optimizer.py:120-192 statement for statement (line numbers in the
comments) with the row sets of all views concatenated.  Nothing of the reference is copied or changed.

    python tools/make_golden_multiview.py

Recorded per iteration: the state (t_obj_cam, code), per-view depth samples, the pooled H, b, dx, the loss, per-view V (size of the first
decode_sdf call inside compute_render_loss) and K (rows it returned; -1 = None), and per-view checksums of the in-sphere and kept sample
sets.  The reference does not expose those sets, so the checksums come from oracle/dsp_oracle.compute_render_loss at the same state and
depths, and are only recorded where its V and K equal the reference's (asserted here).
"""
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim, dsp_oracle as O  # noqa: E402
from dsp_slam_amd import synth, fixtures  # noqa: E402
from tools.make_golden import KITTI, make_cfg  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    ref_shim.install()
    import reconstruct.loss as rloss
    import reconstruct.loss_utils as rlu
    from reconstruct.utils import get_configs, get_decoder

    torch.manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="dsp_fixture_")
    cfg_dict = make_cfg(fixtures.materialize_decoder_dir("cars", os.path.join(tmp, "cars_64")), KITTI)
    with open(os.path.join(tmp, "cfg.json"), "w") as f:
        json.dump(cfg_dict, f)
    decoder = get_decoder(get_configs(os.path.join(tmp, "cfg.json")))
    for p in decoder.parameters():
        p.requires_grad_(False)
    odec = O.fold_decoder(fixtures.load_decoder_npz(fixtures.fixture_path("cars")), fixtures.SPECS)
    j, oc = cfg_dict["optimizer"]["joint_optim"], cfg_dict["optimizer"]
    k1, k2, k3, k4, b1, b2, lr, s_damp = j["k1"], j["k2"], j["k3"], j["k4"], j["b1"], j["b2"], j["learning_rate"], j["scale_damping"]
    code_len, n_depth, th = oc["code_len"], oc["num_depth_samples"], oc["cut_off_threshold"]

    obj = synth.make_object_multiview(31, n_views=3, n_surface=300, n_background=80)
    views = obj["views"]
    real_decode = rloss.decode_sdf
    seen = {}

    def w_dec(dec, z, x, *a, **k):          # the first decode of a compute_render_loss call is over the V in-sphere samples (loss.py:77-78)
        seen.setdefault("V", int(x.shape[0]))
        return real_decode(dec, z, x, *a, **k)

    rloss.decode_sdf = w_dec
    latent_vector = torch.zeros(code_len)                                                    # optimizer.py:96-99
    t_obj_cam = torch.inverse(torch.from_numpy(obj["t_cam_obj_init"].copy()))                # :102-103
    its = []
    loss = 0.
    for e in range(j["num_iterations"]):
        it = dict(t_obj_cam=t_obj_cam.clone().numpy(), code=latent_vector.clone().numpy(), depths=[], V=[], K=[], vsum=[], ksum=[], t_views=[])
        J_s, r_s, J_r, r_r = [], [], [], []
        for v in views:
            # T_oc_v = T_oc T_ref_v: the fp64 product of the two fp32 matrices, rounded once (how the library and the composed oracle define a
            # view's state: one rounding, the same bits everywhere)
            t_v = torch.mm(t_obj_cam.double(), torch.from_numpy(v["t_ref_cam"]).double()).float()
            it["t_views"].append(t_v.clone().numpy())
            t_cam_obj = torch.inverse(t_v)                                                   # :120
            scale = torch.det(t_cam_obj[:3, :3]) ** (1 / 3)                                  # :122
            depth_min, depth_max = t_cam_obj[2, 3] - 1.0 * scale, t_cam_obj[2, 3] + 1.0 * scale
            sampled = torch.linspace(depth_min, depth_max, n_depth)                          # :125
            n_fg = v["depth"].shape[0]
            depth_obs = torch.from_numpy(np.concatenate([v["depth"], np.zeros(v["rays"].shape[0] - n_fg)]).astype(np.float32))
            depth_obs[n_fg:] = 1.1 * depth_max                                               # :126
            a, c, r = rloss.compute_sdf_loss(decoder, torch.from_numpy(v["pts"]), t_v, latent_vector)      # :129
            J_s.append(torch.cat([a, c], dim=-1))
            r_s.append(r)
            seen.clear()
            rend = rloss.compute_render_loss(decoder, torch.from_numpy(v["rays"]), depth_obs, t_v, sampled, latent_vector, th=th)   # :139
            it["depths"].append(sampled.clone().numpy())
            it["V"].append(seen.get("V", 0))
            it["K"].append(-1 if rend is None else int(rend[0].shape[0]))
            st = {}
            orend = O.compute_render_loss(odec, v["rays"], depth_obs.numpy(), t_v.numpy(), sampled.numpy(), latent_vector.numpy(), th=th, stats=st)
            assert st["V"] == it["V"][-1] and (-1 if orend is None else st["K"]) == it["K"][-1], (e, st.get("V"), it["V"][-1], st.get("K"), it["K"][-1])
            it["vsum"].append(0 if orend is None else O.set_checksum(*st["valid"]))
            it["ksum"].append(0 if orend is None else O.set_checksum(*st["kept"]))
            if rend is not None:
                J_r.append(torch.cat([rend[0], rend[1]], dim=-1))
                r_r.append(rend[2])
        J_sdf, res_sdf = torch.cat(J_s, 0), torch.cat(r_s, 0)                                # the views' rows as ONE row set
        J_render, res_render = torch.cat(J_r, 0), torch.cat(r_r, 0)
        robust_res_sdf, sdf_loss, _ = rlu.get_robust_res(res_sdf, b2)                        # :133
        robust_res_render, render_loss, _ = rlu.get_robust_res(res_render, b1)               # :147
        assert not math.isnan(sdf_loss) and not math.isnan(render_loss)
        drot_dsim3, res_rot = rloss.compute_rotation_loss_sim3(t_obj_cam)                    # :153 (the reference camera's frame)
        loss = k1 * render_loss + k2 * sdf_loss                                              # :155
        z = latent_vector.cpu()
        pose_dim = 7
        H_sdf = k2 * torch.bmm(J_sdf.transpose(-2, -1), J_sdf).sum(0).squeeze().cpu() / J_sdf.shape[0]                       # :162
        b_sdf = -k2 * torch.bmm(J_sdf.transpose(-2, -1), robust_res_sdf).sum(0).squeeze().cpu() / J_sdf.shape[0]
        H_render = k1 * torch.bmm(J_render.transpose(-2, -1), J_render).sum(0).squeeze().cpu() / J_render.shape[0]           # :166
        b_render = -k1 * torch.bmm(J_render.transpose(-2, -1), robust_res_render).sum(0).squeeze().cpu() / J_render.shape[0]
        H = H_render + H_sdf
        H[pose_dim:pose_dim + code_len, pose_dim:pose_dim + code_len] += k3 * torch.eye(code_len)                            # :170
        b = b_render + b_sdf
        b[pose_dim:pose_dim + code_len] -= k3 * z                                            # :172
        drot_dsim3 = drot_dsim3.unsqueeze(0)
        H_rot = torch.mm(drot_dsim3.transpose(-2, -1), drot_dsim3)                           # :176
        b_rot = -(drot_dsim3.transpose(-2, -1) * res_rot).squeeze()
        H[:pose_dim, :pose_dim] += k4 * H_rot
        b[:pose_dim] -= k4 * b_rot                                                           # :179
        H[:pose_dim, :pose_dim] += 1e0 * torch.eye(pose_dim)                                 # :183
        H[pose_dim - 1, pose_dim - 1] += s_damp                                              # :184
        dx = torch.mv(torch.inverse(H), b)                                                   # :186
        it.update(H=H.clone().numpy(), b=b.clone().numpy(), dx=dx.clone().numpy(), loss=np.float32(float(loss)))
        its.append(it)
        delta_t = rlu.exp_sim3(lr * dx[:pose_dim])                                           # :190
        t_obj_cam = torch.mm(delta_t, t_obj_cam)                                             # :191
        latent_vector = latent_vector + lr * dx[pose_dim:pose_dim + code_len]                # :192
    rloss.decode_sdf = real_decode
    out = {"it_" + k: np.stack([np.asarray(i[k]) for i in its]).astype(np.float32) for k in ("t_obj_cam", "code", "depths", "H", "b", "dx", "loss", "t_views")}
    for k in ("V", "K", "vsum", "ksum"):
        out["it_" + k] = np.array([i[k] for i in its], np.int64)
    out["t_cam_obj"] = torch.inverse(t_obj_cam).numpy()                                      # :200
    out["code"] = latent_vector.numpy()
    out["loss"] = np.float32(float(loss))
    out["in_t_cam_obj_init"] = obj["t_cam_obj_init"]
    out["in_code_gt"] = obj["code_gt"]
    for n, v in enumerate(views):
        for k in ("t_ref_cam", "pts", "rays", "depth"):
            out["in_v%d_%s" % (n, k)] = v[k]
    cfg_dict["DeepSDF_DIR"] = "cars_64"
    out["cfg_json"] = np.array(json.dumps(cfg_dict))
    path = os.path.join(GOLD, "golden_multiview_cars3.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; V", out["it_V"].tolist(), "K", out["it_K"].tolist(), "loss", out["it_loss"].tolist())


if __name__ == "__main__":
    main()
