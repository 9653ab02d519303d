"""GPU: tools/reoptimise_map.py on a saved map whose objects have several observation files (observations/<id>.npz, <id>.1.npz, ...):
such an object is optimised over all its views -- the same bits as Engine.reconstruct_multiview_batch on the same views -- while an object
with one file, in the same map, gets what reconstruct_batch gives it, and an unobserved object keeps what the map holds."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from dsp_slam_amd import engine as E, synth
from dsp_slam_amd.map_objects import read_map_objects, write_map_objects

pytestmark = pytest.mark.gpu


def test_reoptimise_map_over_all_views(tmp_path, oracle_decoder):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reoptimise_map as R
    map_dir = tmp_path / "map"
    (map_dir / "observations").mkdir(parents=True)
    rng = np.random.default_rng(9)
    objs, made = [], []
    for i, nv in enumerate([3, 1, 2, 0]):
        o = synth.make_object_multiview(80 + i, n_views=max(nv, 1), n_surface=150, n_background=40)
        t_wc = np.eye(4)
        a = rng.uniform(-np.pi, np.pi)
        t_wc[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        t_wc[:3, 3] = rng.uniform(-30, 30, size=3)
        objs.append(dict(id=5 * i + 2, pose=t_wc @ o["t_cam_obj_init"].astype(np.float64), code=np.zeros(64, np.float32)))
        made.append(o)
        for k, v in enumerate(o["views"][:nv]):
            name = "%d.npz" % objs[-1]["id"] if k == 0 else "%d.%d.npz" % (objs[-1]["id"], k)
            np.savez(map_dir / "observations" / name, pts=v["pts"], rays=v["rays"], depth=v["depth"], t_world_cam=t_wc @ v["t_ref_cam"].astype(np.float64))
    write_map_objects(str(map_dir / "MapObjects.txt"), objs)
    objs = read_map_objects(str(map_dir / "MapObjects.txt"))
    obs = R.load_observations(str(map_dir), objs)
    assert [0 if ob is None else 1 + len(ob.get("more_views", [])) for ob in obs] == [3, 1, 2, 0]
    eng = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    prm = E.gn_params(num_iterations=4)
    out, st = R.reoptimise([eng], prm, objs, obs, 64)
    assert st["n_observed"] == 3 and st["n_good"] == 3
    assert np.array_equal(out[3]["pose"], objs[3]["pose"]) and np.array_equal(out[3]["code"], objs[3]["code"])
    # the tool's rows are the library's multi-view results on the views it read
    t_in = [(np.linalg.inv(obs[i]["t_world_cam"]) @ objs[i]["pose"]).astype(np.float32) for i in range(3)]
    direct = eng.reconstruct_multiview_batch(prm, t_in, [R.object_views(obs[i]) for i in range(3)], [np.zeros(64, np.float32)] * 3)
    assert np.array_equal(st["packed"][:, 16:80], direct[1]) and np.array_equal(st["packed"][:, :16].reshape(3, 4, 4), direct[0])
    # the one-file object inside this map: reconstruct_batch's bits
    single = eng.reconstruct_batch(prm, [t_in[1]], [obs[1]["pts"]], [obs[1]["rays"]], [obs[1]["depth"]], [np.zeros(64, np.float32)])
    assert np.array_equal(single[1][0], direct[1][1]) and np.array_equal(single[0][0], direct[0][1])
    # the second and third view were used
    ref_only = eng.reconstruct_batch(prm, [t_in[0]], [obs[0]["pts"]], [obs[0]["rays"]], [obs[0]["depth"]], [np.zeros(64, np.float32)])
    assert not np.array_equal(ref_only[1][0], direct[1][0])
    eng.close()
