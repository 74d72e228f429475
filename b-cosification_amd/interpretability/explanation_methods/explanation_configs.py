"""Named configurations of the explainers that are part of the MI355X hot path (reference
interpretability/explanation_methods/explanation_configs.py:5-30 lists more).  Occlusion -- the one perturbation baseline whose
reference file needs only numpy and torch, so that fixtures could be recorded from it -- runs on the fused engine with the reference's
five named configurations (explanation_configs.py:10-16).  RISE, the second perturbation baseline, runs there too: the one thing its
reference file takes from skimage is a bilinear `resize` with a closed form (include/bcos_hip.h), so its fixtures were recorded from
the reference with that form standing in for skimage.  Its "default" keeps the reference's key "p", which the reference's constructor
swallows (p1 stays 0.1).  LIME and the captum explainers IntGrad, GB, DeepLIFT, GCam stay out of scope: they are comparison methods
whose third-party dependencies (captum, skimage's segmentation) are not available to record the reference from, SURVEY.md section 2
row 12."""

explainer_configs = {
    "Ours": {"default": {}},
    "OursRelative": {"default": {}},
    "IxG": {"default": {}},
    "Grad": {"default": {}},
    "Occlusion": {
        "default": {},
        "Occ5": {"ks": 5, "stride": 2},
        "Occ9": {"ks": 9, "stride": 2},
        "Occ9-TI": {"ks": 9, "stride": 4, "batch_size": 1},
        "Occ13-TI": {"ks": 13, "stride": 4, "batch_size": 1},
    },
    "RISE": {"default": {"n": 500, "s": 8, "p": 0.1, "batch_size": 8}},
}
