"""Training episodes from real volumes, assembled on the device.

`DeviceEpisodeSource.item(idx)` reproduces `FewshotRegReader(mode="train")[idx]` (rpnet_amd/utils/volume_reader.py) —
support volume choice, the elastic coin and field, one random slice per k-block, the intensity coin, gamma and affine
draws, the block shuffle, with the same consumption of the `random` / `numpy.random` / `torch` generators — but keeps the
preprocessed volumes in HBM and does all per-pixel work there: the augmentation kernels of csrc/augment.hip
(rpnet_amd/augment.py) on the k picked slices, then the registration launches (rpnet_amd/registration.py) without their
copies to the host; torch does the plumbing around them (index gathers of the picked slices, the [0,1] maps that feed the
registration, the background mask 1 - fg, concatenation into batches).  After the first use of a volume an item makes no device-to-host copy and no host synchronisation;
what goes up per item is a table of k x 8 parameters, k slice numbers and, when the elastic coin falls, the two noise
planes.  `batch(n)` cuts items into the tuples train_rpnet.train hands to the net.
"""
import random

import numpy as np
import torch

from . import augment as A
from . import registration as R
from .utils.volume_reader import FewshotVolumeReader


class DeviceEpisodeSource:
    """config: the keys of FewshotVolumeReader / FewshotSliceReader (class_csv_dir, train_classes, k, do_elastic,
    do_intaug, gamma_range, do_deformable, crop_size, ...); one way, one shot, `use_registration_loss: True` (what
    FewshotRegReader needs).  `elastic_random_state`: the RandomState of the elastic draws (None: unseeded, as the
    host reader's).  cache_volumes=False reloads a volume every time it is used.  device_load=True builds a volume on the device from
    the payloads of its files (rpnet_amd.volume_load.DeviceVolumeLoader), the same bits as the host reader's.  rank / world: batch() starts at item
    `rank` and strides by `world`, so that the processes of a data-parallel run walk different query volumes."""

    FIELDS = ("support_images", "support_labels", "query_images", "query_labels", "appr_query_labels")

    def __init__(self, data_dir, set_name, config, device, cache_volumes=True, elastic_random_state=None, rank=0, world=1,
                 device_load=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceEpisodeSource runs on MI355X only (there is no CPU fallback; the host reader is "
                               "rpnet_amd.utils.volume_reader.FewshotRegReader)")
        if config["n_way"] != 1 or config["n_shot"] != 1:
            raise NotImplementedError("one way, one shot (the slice reader asserts one way)")
        if not config.get("use_registration_loss", False):
            raise TypeError("DeviceEpisodeSource needs use_registration_loss: True, like FewshotRegReader")
        self.cfg, self.k = config, config["k"]
        self.reader = FewshotVolumeReader(data_dir, set_name, config, mode="train")
        self.cache_volumes, self._volumes = cache_volumes, {}
        self.loader = None
        if device_load:
            from .volume_load import DeviceVolumeLoader
            self.loader = DeviceVolumeLoader(self.reader, self.device)
        self.elastic_random_state = elastic_random_state
        self.pre = None               # the last item's tensors before registration, its slice picks and parameter table
        self.last_elastic = None      # the last item's (Minv, noise), None when the coin fell the other way
        self.world = max(1, int(world))
        self._carry, self._next = None, int(rank) % len(self.reader)

    def __len__(self):
        return len(self.reader)

    def volume(self, c, i):
        """(image [D,H,W], mask [D,H,W]) float32 on the device: the reader's deterministic preprocessing, once"""
        if (c, i) in self._volumes:
            return self._volumes[(c, i)]
        if self.loader is not None:
            v = self.loader.load(self.reader.data_info[c][i]["pid"], self.reader.classes[c])
        else:
            s = self.reader.load_image_and_mask(self.reader.data_info[c][i]["pid"], self.reader.classes[c])
            v = (torch.from_numpy(s["image"][0]).to(self.device), torch.from_numpy(s["mask"][0]).to(self.device))
        if self.cache_volumes:
            self._volumes[(c, i)] = v
        return v

    def warm(self):
        """load every volume and the blur weights of the elastic field (so that no later item copies anything up
        with a blocking copy)"""
        for c, i in self.reader.indices:
            self.volume(c, i)
        A.device_weights(30.0, self.volume(*self.reader.indices[0])[0].device)       # the key elastic_field looks up

    def item(self, idx):
        rd, cfg, dev = self.reader, self.cfg, self.device
        c, qv = rd.indices[idx]
        others = [i for i in range(rd.n_data[c]) if i != qv]
        (s,) = random.choices(others, k=1)
        s_img, s_msk = self.volume(c, s)
        q_img, q_msk = self.volume(c, qv)
        H, W = q_img.shape[-2:]
        elastic = None
        if cfg["do_elastic"] and np.random.randint(2, size=1).item():
            elastic = A.draw_elastic((H, W), random_state=self.elastic_random_state)

        depths = [s_img.shape[0], q_img.shape[0]]
        self.k = k = min([self.k] + depths)                     # sticks for later items, as in the host reader
        n = depths[0]
        s_pick = np.floor(np.arange(n / k / 2, n, n / k)).astype(np.int32)
        nq = depths[1]
        q_edge = np.floor(np.array(np.arange(0, nq, nq / k).tolist() + [nq])).astype(np.int32)
        zs, gammas, affines = [], [], []
        for j in range(k):
            zs.append(int(random.randint(q_edge[j], q_edge[j + 1] - 1)))
            on = cfg["do_intaug"] and np.random.randint(2, size=1).item()
            gammas.append(A.draw_gamma(cfg.get("gamma_range", [0.5, 1.5])) if on else None)
            affines.append(A.draw_random_affine(H, W, **A.TRANSFORM_ARGS))
        order = np.arange(k)
        np.random.shuffle(order)

        # one upload for the three index vectors: query slices, shuffle order, support slices in shuffled order
        idx3 = A.upload(torch.from_numpy(np.stack([np.asarray(zs, np.int64), order.astype(np.int64), s_pick.astype(np.int64)[order]])), dev)
        q, lab = q_img[idx3[0]], q_msk[idx3[0]]
        if elastic is not None:
            q, lab = A.elastic_slices(q, lab, elastic[0], elastic[1])
        params = A.pack_params(affines, gammas)
        q, lab = A.augment_slices(q, lab, params)
        q, lab = q[idx3[1]], lab[idx3[1]]
        sup, sup_l = s_img[idx3[2]], s_msk[idx3[2]]
        if sup.shape != q.shape:
            # make_support_query_same_size would pad here; load_image_and_mask leaves every volume at crop_size, so it never does
            raise NotImplementedError(f"support {tuple(sup.shape)} and query {tuple(q.shape)} slices differ in size")
        self.pre = {"support_images": sup[:, None], "support_labels": sup_l, "query_images": q[:, None], "query_labels": lab,
                    "slices": zs, "order": order, "support_slices": s_pick, "params": params,
                    "affines": affines, "gammas": gammas}
        self.last_elastic = elastic
        pid = rd.data_info[c][qv]["pid"]
        field, reg_pred, _, aff_pred, aff_src = R.register_slices((sup + 1) / 2.0, (q + 1) / 2.0, sup_l,
                                                                   do_deformable=cfg.get("do_deformable", True))
        # reg_pred is already 0 / 1 (thresholded at 0.1 by the warp): the host's `> 0.5` changes nothing
        return {"support_images": aff_src[:, None], "support_labels": aff_pred, "query_images": q[:, None], "query_labels": lab,
                "appr_query_labels": reg_pred, "class_id": c, "registration_field": field, "pid": pid,
                "supp_pids": [(c, s)]}

    def batch(self, n):
        """(si, fg, bg, [qi], ql, appr) of n support/query pairs for RP_Net.forward and the loss: items are drawn in index
        order (from `rank`, stride `world`), round and round, until n pairs are there; what is left over opens the next
        batch."""
        parts = [self._carry] if self._carry is not None else []
        have = sum(p[0].shape[0] for p in parts)
        while have < n:
            it = self.item(self._next)
            self._next = (self._next + self.world) % len(self)
            parts.append([it[f] for f in self.FIELDS])
            have += parts[-1][0].shape[0]
        cat = [torch.cat([p[i] for p in parts]) if len(parts) > 1 else parts[0][i] for i in range(len(self.FIELDS))]
        self._carry = [t[n:] for t in cat] if have > n else None
        si, fg, qi, ql, appr = [t[:n].contiguous() for t in cat]
        return [[si]], [[fg]], [[1.0 - fg]], [qi], ql.long(), appr
