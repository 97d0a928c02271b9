"""Writes tests/golden/onboarding.npz: the reference's OWN helpers run on the case table of tests/onboarding_ref.py (CPU; needs the
reference tree, oracle/refharness.py imports it where it lies).

  get_bbox / get_resize_rgb_choose   Pose_Estimation_Model/utils/data_utils.py (refharness.pem_data_utils())
  CropResizePad                      Instance_Segmentation_Model/utils/bbox_utils.py (refharness.ism().bbox_utils)
  Image.getbbox                      Pillow, on the masks as ``L`` images

Stored: the digest of the inputs (the case table is a pure function of its seed), per view the two boxes, the resized-crop indices of
the defined sampler's picks, and -- for the views whose crop CropResizePad can produce -- the un-normalised template and mask crops
at S = 16.  Regenerates identically (no time stamps, fixed order)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pem_pre as opre  # noqa: E402
from oracle import refharness  # noqa: E402
from tests import onboarding_ref as R  # noqa: E402


def main(out=os.path.join(ROOT, "tests", "golden", "onboarding.npz")):
    from PIL import Image
    du = refharness.pem_data_utils()
    bu = refharness.ism().bbox_utils
    case = R.case_templates()
    views = [i for i in range(R.T) if i != R.EMPTY_VIEW]
    square, rgb_choose, pil = [], [], []
    for i in views:
        mask = case["mask"][i] == 255
        bbox = du.get_bbox(mask)
        square.append([int(v) for v in bbox])
        y1, y2, x1, x2 = square[-1]
        choose = (mask[y1:y2, x1:x2] > 0).astype(np.float32).flatten().nonzero()[0]
        choose = choose[opre.sample_indices(len(choose), R.N_SAMPLE, case["keys"][i])]
        rgb_choose.append(du.get_resize_rgb_choose(choose, bbox, R.S).astype(np.int64))
        pil.append(list(Image.fromarray(case["mask"][i], mode="L").getbbox()))
    assert Image.fromarray(case["mask"][R.EMPTY_VIEW], mode="L").getbbox() is None
    crp = bu.CropResizePad(R.S)
    ism_views, tem, msk = [], [], []
    for i, box in zip(views, pil):
        image = torch.from_numpy(case["rgb"][i] / 255).float()
        m = torch.from_numpy(case["mask"][i] / 255).float()
        image = (image * m[:, :, None]).permute(2, 0, 1)[None]
        b = torch.tensor(np.array([box]))
        try:
            t, k = crp(images=image, boxes=b), crp(images=m[None, None], boxes=b)
        except (AssertionError, RuntimeError):
            continue                                                   # a crop the reference cannot produce
        if tuple(t.shape[-2:]) != (R.S, R.S):
            continue                                                   # ... or one that torch.stack would refuse beside the others
        ism_views.append(i)
        tem.append(t[0].numpy())
        msk.append(k[0, 0].numpy())
    np.savez_compressed(out, digest=np.array(R.digest(case)), views=np.array(views), square=np.array(square, np.int64),
                        rgb_choose=np.stack(rgb_choose), pil=np.array(pil, np.int64), ism_views=np.array(ism_views),
                        templates=np.stack(tem), masks=np.stack(msk))
    print(out, os.path.getsize(out), "bytes; ISM crops for views", ism_views)


if __name__ == "__main__":
    main()
