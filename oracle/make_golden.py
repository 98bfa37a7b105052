"""Generates tests/golden/*.npz by running the REFERENCE's own Python on synthetic inputs.

Run in the build container only (needs /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden
Fixtures hold inputs (or the seeds that regenerate them + a checksum) and the
reference's outputs -- data only, never reference source text.
"""

import os
import sys

import numpy as np
import torch

from foundpose_amd import synthetic
from foundpose_amd.vit_config import VitArch
from oracle import ref_shim

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

TINY = VitArch("tiny-reg", dim=128, depth=3, heads=2, ffn="mlp", hidden=512, registers=4,
               pretrain_grid=4, interp_antialias=True, interp_offset=0.0)


def checksum(*arrays) -> np.float64:
    s = 0.0
    for a in arrays:
        a = np.asarray(a, np.float64).ravel()
        s += float((a * np.cos(np.arange(a.size) * 0.37)).sum())
    return np.float64(s)


def t2n(x):
    return x.detach().cpu().numpy()


# ------------------------------------------------------------------ matching cases
MATCH_CASES = {
    # name: dict(T, pmin, pmax, W, planted template, noise, top_n, top_k, soft, bank_seed, q_seed, dup)
    "match_planted": dict(T=24, pmin=30, pmax=60, W=128, tpl=7, noise=0.05, top_n=5, top_k=300, soft=False, bank_seed=7, q_seed=100, dup=0),
    "match_ties": dict(T=24, pmin=40, pmax=70, W=96, tpl=3, noise=0.0, top_n=5, top_k=300, soft=False, bank_seed=8, q_seed=101, dup=12),
    "match_boundary": dict(T=30, pmin=150, pmax=220, W=256, tpl=11, noise=0.3, top_n=5, top_k=50, soft=False, bank_seed=9, q_seed=102, dup=20),
    "match_soft": dict(T=16, pmin=30, pmax=50, W=64, tpl=5, noise=0.05, top_n=3, top_k=20, soft=True, bank_seed=10, q_seed=103, dup=0),
    "match_partialsort": dict(T=400, pmin=8, pmax=16, W=128, tpl=123, noise=0.05, top_n=5, top_k=300, soft=False, bank_seed=12, q_seed=104, dup=0),
}


def build_match_inputs(c):
    """Deterministic inputs of a matching case (shared by the generator and the tests)."""
    bank = synthetic.make_bank_features(c["T"], 256, c["pmin"], c["pmax"], seed=c["bank_seed"])
    centroids = synthetic.pick_centroids(bank["feat_vectors"], c["W"], seed=c["bank_seed"] + 1000)
    pts, feats = synthetic.make_planted_query(bank, c["tpl"], 37, seed=c["q_seed"], noise=c["noise"])
    if c["dup"]:
        # duplicate some query features at other grid cells -> exact distance ties
        d = c["dup"]
        feats = torch.cat([feats, feats[:d]], 0)
        extra = pts[:d].clone()
        extra[:, 1] = 518.0 - 7.0  # bottom row of the grid, unused by make_planted_query's first rows? keep distinct anyway
        extra[:, 0] = torch.arange(d).float() * 14.0 + 7.0
        pts = torch.cat([pts, extra], 0)
    return bank, centroids, pts.contiguous(), feats.contiguous()


def gen_match(ref):
    for name, c in MATCH_CASES.items():
        bank, centroids, pts, feats = build_match_inputs(c)
        T = c["T"]
        opts = ref.repre_util.TemplateDescOpts(tfidf_soft_assign=c["soft"])
        # word assignment (the k-means 1-NN assignment of the bank builder)
        words_index = ref.knn_util.KNN(k=1, metric="l2")
        words_index.fit(centroids)
        _, wid = words_index.search(bank["feat_vectors"])
        feat_to_cluster_ids = wid[:, 0].to(torch.int32)
        descs, idfs = ref.template_util.calc_tfidf_descriptors(
            feat_vectors=bank["feat_vectors"], feat_to_word_ids=feat_to_cluster_ids,
            feat_to_template_ids=bank["feat_to_template_ids"], feat_words=centroids,
            num_templates=T, tfidf_knn_k=opts.tfidf_knn_k, tfidf_soft_assign=opts.tfidf_soft_assign,
            tfidf_soft_sigma_squared=opts.tfidf_soft_sigma_squared,
        )
        repre = ref.repre_util.FeatureBasedObjectRepre(
            vertices=bank["vertices"], feat_vectors=bank["feat_vectors"],
            feat_to_vertex_ids=bank["feat_to_vertex_ids"], feat_to_template_ids=bank["feat_to_template_ids"],
            feat_to_cluster_ids=feat_to_cluster_ids, feat_cluster_centroids=centroids,
            feat_cluster_idfs=idfs, template_descs=descs, template_desc_opts=opts,
        )
        vw = ref.knn_util.KNN(k=opts.tfidf_knn_k, metric=opts.tfidf_knn_metric)
        vw.fit(centroids)
        tpl_idx = []
        for t in range(T):
            ids = torch.nonzero(bank["feat_to_template_ids"] == t).flatten()
            idx = ref.knn_util.KNN(k=1, metric="l2")
            idx.fit(bank["feat_vectors"][ids])
            tpl_idx.append(idx)
        corresp = ref.corresp_util.establish_correspondences(
            query_points=pts, query_features=feats, object_repre=repre,
            template_matching_type="tfidf", feat_matching_type="cyclic_buddies",
            top_n_templates=c["top_n"], top_k_buddies=c["top_k"],
            visual_words_knn_index=vw, template_knn_indices=tpl_idx, debug=True,
        )
        out = {
            "input_checksum": checksum(bank["feat_vectors"], centroids, pts, feats),
            "feat_to_cluster_ids": t2n(feat_to_cluster_ids),
            "word_idfs": t2n(idfs), "template_descs": t2n(descs),
            "template_ids": np.array([int(cc["template_id"]) for cc in corresp], np.int64),
            "template_scores": np.array([float(cc["template_score"]) for cc in corresp], np.float32),
        }
        for i, cc in enumerate(corresp):
            out[f"coord_2d_ids_{i}"] = t2n(cc["coord_2d_ids"]).astype(np.int64)
            out[f"nn_vertex_ids_{i}"] = t2n(cc["nn_vertex_ids"]).astype(np.int64)
            out[f"coord_conf_{i}"] = t2n(cc["coord_conf"]).astype(np.float32)
            out[f"coord_2d_{i}"] = t2n(cc["coord_2d"]).astype(np.float32)
            out[f"coord_3d_{i}"] = t2n(cc["coord_3d"]).astype(np.float32)
            out[f"nn_dists_{i}"] = t2n(cc["nn_dists"]).astype(np.float32)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
        print(name, "templates", out["template_ids"], "k", [len(out[f'coord_2d_ids_{i}']) for i in range(len(corresp))])


# ------------------------------------------------------------------ point utils / sampling / PCA
def gen_points(ref):
    fu, pu = ref.feature_util, ref.projector_util
    out = {}
    for s in (518, 420):
        out[f"grid_{s}"] = t2n(fu.generate_grid_points((s, s), 14.0))
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand(518, 518, generator=g) > 0.6).to(torch.uint8)
    pts = fu.generate_grid_points((518, 518), 14.0)
    out["mask_seed"] = np.int64(5)
    out["filtered_random"] = t2n(fu.filter_points_by_mask(pts, mask))
    out["filtered_disc"] = t2n(fu.filter_points_by_mask(pts, synthetic.make_disc_mask(518)))
    fmap = torch.randn(48, 37, 37, generator=g)
    qp = fu.filter_points_by_mask(pts, synthetic.make_disc_mask(518))
    offgrid = torch.rand(64, 2, generator=g) * 518.0
    out["fmap"] = t2n(fmap)
    out["offgrid_points"] = t2n(offgrid)
    out["sampled_grid"] = t2n(fu.sample_feature_map_at_points(fmap, qp, (518, 518)))
    out["sampled_offgrid"] = t2n(fu.sample_feature_map_at_points(fmap, offgrid, (518, 518)))
    # PCA: fit through the reference projector (sklearn), then transform.
    x = torch.randn(600, 48, generator=g) * torch.linspace(2.0, 0.2, 48) + torch.linspace(-1, 1, 48)
    proj = pu.PCAProjector(n_components=16)
    proj.fit(x)
    td = pu.projector_to_tensordict(proj)["pca_projector"]
    proj2 = pu.projector_from_tensordict({"pca_projector": td})
    y = pu.project_features(x[:100], [proj2])
    out["pca_x"] = t2n(x[:100])
    out["pca_components"] = t2n(td["components"]).astype(np.float32)
    out["pca_mean"] = t2n(td["mean"]).astype(np.float32)
    out["pca_y"] = t2n(y).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "points_sample_pca.npz"), **out)
    print("points_sample_pca", {k: np.asarray(v).shape for k, v in out.items()})


# ------------------------------------------------------------------ extractor wrapper
def _make_ref_extractor(ref, arch, sd, image_size, name):
    base = f"dinov2_{arch.name}".replace("-", "_")
    ref_shim.set_backbone(base, lambda pretrained=True: ref_shim.HFBackboneAdapter(sd, arch, image_size))
    return ref.dinov2_utils.DinoFeatureExtractor(name)


def gen_extractor(ref):
    from foundpose_amd.vit_config import ARCHS

    ARCHS[TINY.name] = TINY
    # (a) tiny architecture, full outputs, two layers, with and without the final norm
    sd = synthetic.make_vit_state_dict(TINY, seed=1234)
    imgs = synthetic.make_crops(2, 56, seed=0)
    out = {"weights_seed": np.int64(1234), "image_seed": np.int64(0),
           "input_checksum": checksum(imgs, sd["blocks.1.attn.qkv.weight"], sd["pos_embed"])}
    for layer, norm in ((1, 1), (2, 1), (0, 0)):
        ex = _make_ref_extractor(ref, TINY, sd, 56, f"dinov2_version=tiny-reg_stride=14_facet=token_layer={layer}_logbin=0_norm={norm}")
        with torch.no_grad():
            o = ex(imgs)
        out[f"fmap_l{layer}_n{norm}"] = t2n(o["feature_maps"]).astype(np.float32)
        out[f"cls_l{layer}_n{norm}"] = t2n(o["cls_tokens"]).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "extractor_tiny.npz"), **out)
    print("extractor_tiny", out["fmap_l1_n1"].shape)

    # (a') key / query / value facets through the reference wrapper's attention hooks (dinov2_utils.py:176-194)
    fac = {"weights_seed": np.int64(1234), "image_seed": np.int64(0)}
    for facet in ("key", "query", "value"):
        for layer, norm in ((1, 1), (2, 0)):
            ex = _make_ref_extractor(ref, TINY, sd, 56, f"dinov2_version=tiny-reg_stride=14_facet={facet}_layer={layer}_logbin=0_norm={norm}")
            with torch.no_grad():
                o = ex(imgs)
            fac[f"fmap_{facet}_l{layer}_n{norm}"] = t2n(o["feature_maps"]).astype(np.float32)
            fac[f"cls_{facet}_l{layer}_n{norm}"] = t2n(o["cls_tokens"]).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "extractor_tiny_facets.npz"), **fac)
    print("extractor_tiny_facets", fac["fmap_key_l1_n1"].shape)

    # (b) ViT-S/14-reg at 518 (no pos-embed interpolation), the shipped LM-O extractor name.
    arch = ARCHS["vits14-reg"]
    sd = synthetic.make_vit_state_dict(arch, seed=1234)
    imgs = synthetic.make_crops(1, 518, seed=1)
    ex = _make_ref_extractor(ref, arch, sd, 518, "dinov2_version=vits14-reg_stride=14_facet=token_layer=9_logbin=0_norm=1")
    with torch.no_grad():
        o = ex(imgs)
    fm = t2n(o["feature_maps"]).astype(np.float32)
    np.savez_compressed(
        os.path.join(OUT, "extractor_vits14reg_518.npz"),
        weights_seed=np.int64(1234), image_seed=np.int64(1),
        input_checksum=checksum(imgs, sd["blocks.9.attn.qkv.weight"]),
        fmap_sub=fm[:, ::8, ::3, ::3], cls=t2n(o["cls_tokens"]).astype(np.float32),
        fmap_mean=np.float64(fm.mean()), fmap_abs_mean=np.float64(np.abs(fm).mean()),
    )
    print("extractor_vits14reg_518", fm.shape, float(np.abs(fm).mean()))


def gen_extractor_420(ref):
    """(c) ViT-S/14-reg at 420 x 420 -- the reference's shipped LM-O geometry (configs/infer/lmo.json:6-12) -- where the 37 x 37 pos-embed
    table is interpolated to 30 x 30.  The `-reg` hub entries run upstream's interpolate_pos_encoding with interpolate_antialias=True
    and interpolate_offset=0.0, i.e. F.interpolate(size=(30, 30), mode="bicubic", antialias=True); the stand-in backbone
    (transformers' Dinov2WithRegisters, config image_size 518 = the table) interpolates with exactly those arguments, so this
    fixture pins the interpolated table as well as the wrapper."""
    from foundpose_amd.vit_config import ARCHS
    arch = ARCHS["vits14-reg"]
    sd = synthetic.make_vit_state_dict(arch, seed=1234)
    imgs = synthetic.make_crops(1, 420, seed=3)
    ex = _make_ref_extractor(ref, arch, sd, 518, "dinov2_version=vits14-reg_stride=14_facet=token_layer=9_logbin=0_norm=1")
    with torch.no_grad():
        o = ex(imgs)
    fm = t2n(o["feature_maps"]).astype(np.float32)
    assert fm.shape == (1, 384, 30, 30)
    np.savez_compressed(
        os.path.join(OUT, "extractor_vits14reg_420.npz"),
        weights_seed=np.int64(1234), image_seed=np.int64(3),
        input_checksum=checksum(imgs, sd["blocks.9.attn.qkv.weight"], sd["pos_embed"]),
        fmap_sub=fm[:, ::4, ::2, ::2], cls=t2n(o["cls_tokens"]).astype(np.float32),
        fmap_mean=np.float64(fm.mean()), fmap_abs_mean=np.float64(np.abs(fm).mean()),
    )
    print("extractor_vits14reg_420", fm.shape, float(np.abs(fm).mean()))


def gen_extractor_stride(ref):
    """(d) stride != patch size.  The reference's own branch cannot run end to end: `_fix_pos_enc` returns a function declared
    without `self` that closes over the WRAPPER's (non-existent) pos_embed and is bound with types.MethodType (dinov2_utils.py:325-326,386-388).
    What its code states is still executable piece by piece, and that is what this fixture pins: the reference's position-encoding function
    itself (called on an object that has the table), the reference wrapper's constructor (it sets the conv stride of the backbone) and forward
    (hook, token slicing, 1 + (size - patch) // stride grid, final norm), over the stand-in backbone whose embedding calls that function."""
    import types as _types
    from foundpose_amd.vit_config import ARCHS
    ARCHS[TINY.name] = TINY
    sd = synthetic.make_vit_state_dict(TINY, seed=1234)
    fn = ref.dinov2_utils.DinoFeatureExtractor._fix_pos_enc(_types.SimpleNamespace(pos_embed=sd["pos_embed"]), TINY.patch, (7, 7))
    out = {"weights_seed": np.int64(1234), "image_seed": np.int64(0), "stride": np.int64(7)}
    for (H, W) in ((56, 56), (70, 56), (28, 28)):
        npatch = (1 + (H - 14) // 7) * (1 + (W - 14) // 7)
        out[f"pos_{H}x{W}"] = t2n(fn(torch.zeros(1, 1 + npatch, TINY.dim), H, W)).astype(np.float32)   # upstream passes (x, image height, image width)
    imgs = synthetic.make_crops(2, 56, seed=0)
    for layer, norm in ((2, 1), (0, 0)):
        ex = _make_ref_extractor(ref, TINY, sd, 56, f"dinov2_version=tiny-reg_stride=7_facet=token_layer={layer}_logbin=0_norm={norm}")
        assert ex.stride == 7 and tuple(ex.model.patch_embed.proj.stride) == (7, 7)
        ex.model.hf.embeddings.interpolate_pos_encoding = lambda emb, height, width: fn(emb, height, width)
        with torch.no_grad():
            o = ex(imgs)
        out[f"fmap_l{layer}_n{norm}"] = t2n(o["feature_maps"]).astype(np.float32)
        out[f"cls_l{layer}_n{norm}"] = t2n(o["cls_tokens"]).astype(np.float32)
    assert out["fmap_l2_n1"].shape == (2, TINY.dim, 7, 7)
    np.savez_compressed(os.path.join(OUT, "extractor_tiny_stride7.npz"), **out)
    print("extractor_tiny_stride7", out["fmap_l2_n1"].shape, out["pos_70x56"].shape)


TINY0 = VitArch("tiny", dim=128, depth=3, heads=2, ffn="mlp", hidden=512, registers=0,
                pretrain_grid=4, interp_antialias=False, interp_offset=0.1)


def gen_extractor_noreg(ref):
    """(e) the NON-register hub entries -- `InferOpts.extractor_name` defaults to "dinov2_vitl14" (scripts/infer.py:75; short form: layer
    stays 9, dinov2_utils.py:62-64; hub name dinov2_utils.py:81-84).  0 register tokens (the wrapper drops 1 + 0 prefix rows,
    dinov2_utils.py:304) and, off 518 x 518, upstream's scale-factor pos-embed interpolation with the +0.1 offset and no antialias.
    The stand-in backbone is transformers' Dinov2Model carrying the same weights; its size-mode interpolation is replaced by the
    REFERENCE's own `_fix_pos_enc(patch, (patch, patch))` function (dinov2_utils.py:325-360), which at stride = patch is upstream's
    offset branch argument for argument: F.interpolate(scale_factor=((w0 + .1)/M, (h0 + .1)/M), bicubic, no antialias)."""
    import types as _types
    from foundpose_amd.vit_config import ARCHS

    ARCHS[TINY0.name] = TINY0

    def make(arch, sd, name):
        fn = ref.dinov2_utils.DinoFeatureExtractor._fix_pos_enc(_types.SimpleNamespace(pos_embed=sd["pos_embed"]), arch.patch, (arch.patch, arch.patch))
        base = f"dinov2_{arch.name}".replace("-", "_")
        ref_shim.set_backbone(base, lambda pretrained=True: ref_shim.HFBackboneAdapter(sd, arch, arch.pretrain_grid * arch.patch, pos_fn=fn))
        ex = ref.dinov2_utils.DinoFeatureExtractor(name)
        assert ex.model.num_register_tokens == 0
        return ex, fn

    # tiny: full outputs; the native grid (no interpolation), a larger square grid, a non-square one
    sd = synthetic.make_vit_state_dict(TINY0, seed=1234)
    out = {"weights_seed": np.int64(1234), "image_seed": np.int64(0)}
    for (H, W) in ((56, 56), (84, 84), (70, 42)):
        g = torch.Generator().manual_seed(H * 1000 + W)
        imgs = torch.rand(2, 3, H, W, generator=g)
        for layer, norm in ((2, 1), (0, 0)):
            ex, fn = make(TINY0, sd, f"dinov2_version=tiny_stride=14_facet=token_layer={layer}_logbin=0_norm={norm}")
            with torch.no_grad():
                o = ex(imgs)
            out[f"fmap_{H}x{W}_l{layer}_n{norm}"] = t2n(o["feature_maps"]).astype(np.float32)
            out[f"cls_{H}x{W}_l{layer}_n{norm}"] = t2n(o["cls_tokens"]).astype(np.float32)
        out[f"pos_{H}x{W}"] = t2n(fn(torch.zeros(1, 1 + (H // 14) * (W // 14), TINY0.dim), H, W)).astype(np.float32)
    assert out["fmap_70x42_l2_n1"].shape == (2, TINY0.dim, 5, 3)
    np.savez_compressed(os.path.join(OUT, "extractor_tiny_noreg.npz"), **out)
    print("extractor_tiny_noreg", out["fmap_84x84_l2_n1"].shape, out["pos_70x42"].shape)

    # the hub architectures through their SHORT names (layer 9) and one long name; 518 (table as is) and 420 (LM-O crop size)
    cases = (("vitl14", "dinov2_vitl14", 518, 8, 3), ("vitl14", "dinov2_vitl14", 420, 8, 2),
             ("vits14", "dinov2_vits14", 420, 4, 2), ("vitb14", "dinov2_vitb14", 518, 8, 3),
             ("vitb14", "dinov2_version=vitb14_stride=14_facet=token_layer=11_norm=1", 420, 8, 2),
             ("vitg14", "dinov2_vitg14", 224, 16, 1))    # BASELINE config 5's "ViT-g/14" without registers: SwiGLU FFN, 24 heads, interpolated table
    for version, name, S, cs, ss in cases:
        arch = ARCHS[version]
        sd = synthetic.make_vit_state_dict(arch, seed=1234)
        imgs = synthetic.make_crops(1, S, seed=5)
        ex, _ = make(arch, sd, name)
        assert ex.layer == (11 if "layer=11" in name else 9)
        with torch.no_grad():
            o = ex(imgs)
        fm = t2n(o["feature_maps"]).astype(np.float32)
        assert fm.shape == (1, arch.dim, S // 14, S // 14)
        np.savez_compressed(
            os.path.join(OUT, f"extractor_{version}_{S}.npz"),
            weights_seed=np.int64(1234), image_seed=np.int64(5), layer=np.int64(ex.layer), name=np.array(name),
            input_checksum=checksum(imgs, sd[f"blocks.{ex.layer}.attn.qkv.weight"], sd["pos_embed"]),
            fmap_sub=fm[:, ::cs, ::ss, ::ss], cls=t2n(o["cls_tokens"]).astype(np.float32), sub=np.array([cs, ss]),
            fmap_mean=np.float64(fm.mean()), fmap_abs_mean=np.float64(np.abs(fm).mean()),
        )
        print(f"extractor_{version}_{S}", fm.shape, float(np.abs(fm).mean()))


# ------------------------------------------------------------------ composite hot section
def gen_hot_section(ref):
    """infer.py:468-542 driven through the reference's functions on a tiny extractor."""
    from foundpose_amd.vit_config import ARCHS

    ARCHS[TINY.name] = TINY
    fu, pu = ref.feature_util, ref.projector_util
    S, cell = 112, 14.0  # 8x8 patch grid; pos-embed interpolated from the 4x4 table
    sd = synthetic.make_vit_state_dict(TINY, seed=77)
    # HF interpolates its 4x4 table to 8x8 itself (size-based, antialias): same flavour as the -reg hub models.
    ex = _make_ref_extractor(ref, TINY, sd, 56, "dinov2_version=tiny-reg_stride=14_facet=token_layer=2_logbin=0_norm=1")
    g = torch.Generator().manual_seed(42)
    T = 12
    tpl_imgs = torch.rand(T, 3, S, S, generator=g)
    tpl_masks = (torch.rand(T, S, S, generator=g) > 0.35).to(torch.uint8)
    grid = fu.generate_grid_points((S, S), cell)
    feats, f2t, verts = [], [], []
    with torch.no_grad():
        for t in range(T):
            fm = ex(tpl_imgs[t:t + 1])["feature_maps"][0]
            qp = fu.filter_points_by_mask(grid, tpl_masks[t])
            feats.append(fu.sample_feature_map_at_points(fm, qp, (S, S)).contiguous())
            f2t.append(torch.full((len(qp),), t, dtype=torch.int32))
            verts.append(torch.cat([qp, torch.full((len(qp), 1), float(t))], 1))
    raw = torch.cat(feats, 0)
    f2t = torch.cat(f2t)
    verts = torch.cat(verts, 0)
    proj = pu.PCAProjector(n_components=32)
    proj.fit(raw)
    td = pu.projector_to_tensordict(proj)["pca_projector"]
    proj = pu.projector_from_tensordict({"pca_projector": td})
    bank_feats = pu.project_features(raw, [proj]).contiguous()
    W = 48
    centroids = synthetic.pick_centroids(bank_feats, W, seed=3)
    opts = ref.repre_util.TemplateDescOpts()
    k1 = ref.knn_util.KNN(k=1, metric="l2"); k1.fit(centroids)
    f2c = k1.search(bank_feats)[1][:, 0].to(torch.int32)
    descs, idfs = ref.template_util.calc_tfidf_descriptors(
        bank_feats, f2c, f2t, centroids, T, opts.tfidf_knn_k, opts.tfidf_soft_assign, opts.tfidf_soft_sigma_squared)
    repre = ref.repre_util.FeatureBasedObjectRepre(
        vertices=verts, feat_vectors=bank_feats, feat_to_vertex_ids=torch.arange(len(verts), dtype=torch.int32),
        feat_to_template_ids=f2t, feat_to_cluster_ids=f2c, feat_cluster_centroids=centroids,
        feat_cluster_idfs=idfs, template_descs=descs, template_desc_opts=opts, feat_raw_projectors=[proj])
    vw = ref.knn_util.KNN(k=3, metric="l2"); vw.fit(centroids)
    tpl_idx = []
    for t in range(T):
        idx = ref.knn_util.KNN(k=1, metric="l2"); idx.fit(bank_feats[f2t == t]); tpl_idx.append(idx)
    # query = template 4 + noise, its own mask
    q_img = (tpl_imgs[4] + 0.02 * torch.randn(3, S, S, generator=g)).clamp(0, 1)
    q_mask = tpl_masks[4]
    with torch.no_grad():
        fmap = ex(q_img.unsqueeze(0))["feature_maps"][0]
        qp = fu.filter_points_by_mask(grid, q_mask)
        qf = fu.sample_feature_map_at_points(fmap, qp, (S, S)).contiguous()
        qfp = pu.project_features(qf, repre.feat_raw_projectors).contiguous()
        corresp = ref.corresp_util.establish_correspondences(
            query_points=qp, query_features=qfp, object_repre=repre, template_matching_type="tfidf",
            feat_matching_type="cyclic_buddies", top_n_templates=5, top_k_buddies=300,
            visual_words_knn_index=vw, template_knn_indices=tpl_idx, debug=True)
    out = dict(
        weights_seed=np.int64(77), data_seed=np.int64(42), image_size=np.int64(S),
        tpl_imgs=(t2n(tpl_imgs) * 255).round().astype(np.uint8) if False else t2n(tpl_imgs).astype(np.float16),
        tpl_masks=t2n(tpl_masks), q_img=t2n(q_img).astype(np.float32),
        pca_components=t2n(td["components"]).astype(np.float32), pca_mean=t2n(td["mean"]).astype(np.float32),
        bank_feats=t2n(bank_feats).astype(np.float32), f2t=t2n(f2t), vertices=t2n(verts).astype(np.float32),
        centroids=t2n(centroids).astype(np.float32), idfs=t2n(idfs), template_descs=t2n(descs),
        fmap=t2n(fmap).astype(np.float32), query_points=t2n(qp), query_features=t2n(qf), query_features_proj=t2n(qfp),
        template_ids=np.array([int(c["template_id"]) for c in corresp], np.int64),
        template_scores=np.array([float(c["template_score"]) for c in corresp], np.float32),
    )
    for i, c in enumerate(corresp):
        out[f"coord_2d_ids_{i}"] = t2n(c["coord_2d_ids"]).astype(np.int64)
        out[f"nn_vertex_ids_{i}"] = t2n(c["nn_vertex_ids"]).astype(np.int64)
        out[f"coord_conf_{i}"] = t2n(c["coord_conf"]).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "hot_section_tiny.npz"), **out)
    print("hot_section_tiny", out["template_ids"], out["template_scores"], "Q", len(qp))


def gen_crop(ref):
    """Crop producer: crop box, virtual crop camera and the fp32 destination->source maps, from the reference's own
    utils/misc.py (calc_crop_box, construct_crop_camera, warp_image) with a cv2.remap stand-in that captures the maps."""
    import importlib
    structs = importlib.import_module("utils.structs")
    captured = {}

    def capture(src, map_x, map_y, interpolation):
        captured["map"] = (np.array(map_x), np.array(map_y))
        return np.zeros(map_x.shape + src.shape[2:], dtype=src.dtype)

    sys.modules["cv2"].remap = capture
    rng = np.random.default_rng(11)

    def rigid(angle_deg, axis, t):
        a = np.asarray(axis, dtype=np.float64)
        a /= np.linalg.norm(a)
        th = np.deg2rad(angle_deg)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        T = np.eye(4)
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        T[:3, 3] = t
        return T

    cases = [  # (name, width, height, f, c, T_world_from_eye, box ltrb, viewport, rel_pad)
        ("lmo", 640, 480, (572.4114, 573.57043), (325.2611, 242.04899), np.eye(4), (250.0, 140.0, 380.0, 300.0), (56, 56), 0.2),
        ("edge", 640, 480, (572.4114, 573.57043), (325.2611, 242.04899), rigid(33.0, (0.2, 1.0, -0.3), (0.1, -0.4, 1.2)),
         (-20.0, 400.0, 90.0, 470.0), (56, 56), 0.2),
        ("wide", 1920, 1080, (1066.778, 1067.487), (312.9869 + 640, 241.3109 + 300), rigid(-71.0, (1.0, 0.1, 0.4), (3.0, 0.2, -0.7)),
         (900.0, 200.0, 1700.0, 520.0), (518, 518), 0.2),
        ("tiny", 640, 480, (572.4114, 573.57043), (325.2611, 242.04899), rigid(5.0, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)),
         (300.0, 200.0, 312.0, 230.0), (420, 420), 0.5),
    ]
    out = {"names": np.array([c[0] for c in cases])}
    for name, w, h, f, c, T, box, vp, pad in cases:
        cam = structs.PinholePlaneCameraModel(width=w, height=h, f=f, c=c, T_world_from_eye=T)
        b = structs.AlignedBox2f(left=box[0], top=box[1], right=box[2], bottom=box[3])
        cb = ref.misc.calc_crop_box(box=b, make_square=True)
        cc = ref.misc.construct_crop_camera(box=cb, camera_model_c2w=cam, viewport_size=vp, viewport_rel_pad=pad)
        ref.misc.warp_image(src_camera=cam, dst_camera=cc, src_image=np.zeros((h, w, 3), np.float32), interpolation=1)
        mx, my = captured["map"]
        rows = slice(None) if vp[0] <= 64 else slice(None, None, 37)
        out.update({f"{name}_cam": np.array([w, h, *f, *c], dtype=np.float64), f"{name}_T": np.array(T),
                    f"{name}_box": np.array(box), f"{name}_vp": np.array(vp), f"{name}_pad": np.float64(pad),
                    f"{name}_crop_box": np.array([cb.left, cb.top, cb.right, cb.bottom]),
                    f"{name}_crop_f": np.array(cc.f, dtype=np.float64), f"{name}_crop_c": np.array(cc.c, dtype=np.float64),
                    f"{name}_crop_T": np.array(cc.T_world_from_eye), f"{name}_map_x": mx[rows], f"{name}_map_y": my[rows],
                    f"{name}_map_sum": checksum(mx, my)})
    # depth check: a destination camera turned 120 degrees away from the source sees rays behind it -> -1
    src = structs.PinholePlaneCameraModel(width=320, height=240, f=(300.0, 300.0), c=(159.5, 119.5), T_world_from_eye=np.eye(4))
    dst = structs.PinholePlaneCameraModel(width=48, height=40, f=(np.float32(20.0), np.float32(20.0)), c=(np.float32(23.5), np.float32(19.5)),
                                          T_world_from_eye=rigid(80.0, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)))
    ref.misc.warp_image(src_camera=src, dst_camera=dst, src_image=np.zeros((240, 320), np.uint8), interpolation=0)
    out.update({"behind_map_x": captured["map"][0], "behind_map_y": captured["map"][1], "behind_dst_T": dst.T_world_from_eye})
    np.savez_compressed(os.path.join(OUT, "crop_camera.npz"), **out)
    print("crop_camera.npz", {k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items() if k.endswith("map_x")})


def gen_lift(ref):
    """feature_util.lift_2d_points_to_3d + geometry.transform_3d_points_torch of the reference on a synthetic depth map."""
    import importlib
    structs = importlib.import_module("utils.structs")
    geometry = importlib.import_module("utils.geometry")
    g = torch.Generator().manual_seed(21)
    S = 84
    depth = 400.0 + 100.0 * torch.rand(S, S, generator=g)
    cam = structs.PinholePlaneCameraModel(width=S, height=S, f=(131.7, 129.3), c=(41.2, 40.6), T_world_from_eye=np.eye(4))
    grid = ref.feature_util.generate_grid_points((S, S), 14.0)
    mask = torch.zeros(S, S, dtype=torch.uint8)
    mask[10:70, 5:80] = 1
    pts = ref.feature_util.filter_points_by_mask(grid, mask)
    v_cam = ref.feature_util.lift_2d_points_to_3d(points=pts, depth_image=depth, camera_model=cam)
    T = torch.eye(4)
    T[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    T[:3, 3] = torch.tensor([12.0, -7.5, 310.0])
    v_model = geometry.transform_3d_points_torch(T, v_cam)
    np.savez_compressed(os.path.join(OUT, "lift_3d.npz"), depth=t2n(depth), mask=t2n(mask), points=t2n(pts), cam=np.array([131.7, 129.3, 41.2, 40.6]),
                        T=t2n(T), vertices_in_cam=t2n(v_cam), vertices_in_model=t2n(v_model))
    print("lift_3d.npz", v_model.shape)


WRAP = dict(T=12, d=64, pmin=20, pmax=30, W=32, raw=96, tpl=5, bank_seed=31, q_seed=33)


def build_wrapper_inputs():
    """Deterministic inputs of the row-R / wrapper fixture (shared by the generator and the tests)."""
    c = WRAP
    bank = synthetic.make_bank_features(c["T"], c["d"], c["pmin"], c["pmax"], seed=c["bank_seed"])
    centroids = synthetic.pick_centroids(bank["feat_vectors"], c["W"], seed=c["bank_seed"] + 1)
    pts, feats = synthetic.make_planted_query(bank, c["tpl"], 37, seed=c["q_seed"], noise=0.05)
    g = torch.Generator().manual_seed(c["q_seed"] + 1)
    raw_train = torch.randn(400, c["raw"], generator=g) * (torch.arange(1, c["raw"] + 1, dtype=torch.float32) ** -0.5)
    raw_query = torch.randn(pts.shape[0], c["raw"], generator=g)
    return bank, centroids, pts.contiguous(), feats.contiguous(), raw_train, raw_query


def gen_wrappers(ref):
    """Row R and the standalone wrappers: a `repre.pth` written by the reference's own save_object_repre (a data file:
    tensors, option dicts, camera dicts) and the outputs of the reference's find_nearest_object_features, calc_tfidf,
    tfidf_matching, cyclic_buddies_matching, KNN(metric="cosine"), PCAProjector.transform and establish_correspondences
    on the representation its load_object_repre reads back."""
    import importlib
    structs = importlib.import_module("utils.structs")
    c = WRAP
    bank, centroids, pts, feats, raw_train, raw_query = build_wrapper_inputs()
    T = c["T"]
    opts = ref.repre_util.TemplateDescOpts()
    words_index = ref.knn_util.KNN(k=1, metric="l2")
    words_index.fit(centroids)
    f2c = words_index.search(bank["feat_vectors"])[1][:, 0].to(torch.int32)
    descs, idfs = ref.template_util.calc_tfidf_descriptors(
        feat_vectors=bank["feat_vectors"], feat_to_word_ids=f2c, feat_to_template_ids=bank["feat_to_template_ids"], feat_words=centroids,
        num_templates=T, tfidf_knn_k=opts.tfidf_knn_k, tfidf_soft_assign=opts.tfidf_soft_assign, tfidf_soft_sigma_squared=opts.tfidf_soft_sigma_squared)
    proj = ref.projector_util.PCAProjector(n_components=c["d"])
    proj.fit(raw_train)
    g = torch.Generator().manual_seed(77)
    cams = []
    for t in range(T):
        Tw = np.eye(4)
        Tw[:3, :3] = np.linalg.qr(torch.randn(3, 3, generator=g).numpy().astype(np.float64))[0]
        Tw[:3, 3] = [10.0 * t, -5.0, 400.0 + t]
        cams.append(structs.PinholePlaneCameraModel(width=420, height=420, f=(600.0 + t, 601.0), c=(210.0, 209.5), T_world_from_eye=Tw))
    repre = ref.repre_util.FeatureBasedObjectRepre(
        vertices=bank["vertices"], feat_vectors=bank["feat_vectors"], feat_opts=ref.repre_util.FeatureOpts(extractor_name="dinov2_vits14-reg"),
        feat_to_vertex_ids=bank["feat_to_vertex_ids"], feat_to_template_ids=bank["feat_to_template_ids"], feat_to_cluster_ids=f2c,
        feat_cluster_centroids=centroids, feat_cluster_idfs=idfs, feat_raw_projectors=[proj], feat_vis_projectors=[],
        template_cameras_cam_from_model=cams, template_descs=descs, template_desc_opts=opts)
    rdir = os.path.join(OUT, "repre_ref")
    os.makedirs(rdir, exist_ok=True)
    ref.repre_util.save_object_repre(repre, rdir)
    loaded = ref.repre_util.load_object_repre(rdir, tensor_device="cpu")

    vw = ref.knn_util.KNN(k=opts.tfidf_knn_k, metric=opts.tfidf_knn_metric)
    vw.fit(loaded.feat_cluster_centroids)
    word_ids, word_dists = ref.template_util.find_nearest_object_features(query_features=feats, knn_index=vw)
    tfidf_hard = ref.template_util.calc_tfidf(word_ids, word_dists, loaded.feat_cluster_idfs, soft_assignment=False, soft_sigma_squared=10.0)
    tfidf_soft = ref.template_util.calc_tfidf(word_ids, word_dists, loaded.feat_cluster_idfs, soft_assignment=True, soft_sigma_squared=10.0)
    tm_ids, tm_scores = ref.template_util.tfidf_matching(feats, loaded, 5, vw)
    tpl_rows = torch.nonzero(loaded.feat_to_template_ids == c["tpl"]).flatten()
    obj_feats = loaded.feat_vectors[tpl_rows]
    q_index, o_index = ref.knn_util.KNN(k=1, metric="l2"), ref.knn_util.KNN(k=1, metric="l2")
    q_index.fit(feats)
    o_index.fit(obj_feats)
    cb = ref.corresp_util.cyclic_buddies_matching(query_points=pts, query_features=feats, query_knn_index=q_index,
                                                  object_features=obj_feats, object_knn_index=o_index, top_k=10, debug=False)
    cos = ref.knn_util.KNN(k=3, metric="cosine")
    cos.fit(loaded.feat_vectors)
    cos_d, cos_i = cos.search(feats)
    projected = ref.projector_util.project_features(raw_query, loaded.feat_raw_projectors)
    tpl_idx = []
    for t in range(T):
        idx = ref.knn_util.KNN(k=1, metric="l2")
        idx.fit(loaded.feat_vectors[torch.nonzero(loaded.feat_to_template_ids == t).flatten()])
        tpl_idx.append(idx)
    corresp = ref.corresp_util.establish_correspondences(
        query_points=pts, query_features=feats, object_repre=loaded, template_matching_type="tfidf", feat_matching_type="cyclic_buddies",
        top_n_templates=5, top_k_buddies=300, visual_words_knn_index=vw, template_knn_indices=tpl_idx, debug=True)
    out = {
        "input_checksum": checksum(bank["feat_vectors"], centroids, pts, feats, raw_train, raw_query),
        "word_ids": t2n(word_ids).astype(np.int64), "word_dists": t2n(word_dists), "tfidf_hard": t2n(tfidf_hard), "tfidf_soft": t2n(tfidf_soft),
        "tm_ids": t2n(tm_ids).astype(np.int64), "tm_scores": t2n(tm_scores),
        "cb_query_ids": t2n(cb[0]).astype(np.int64), "cb_object_ids": t2n(cb[1]).astype(np.int64), "cb_dists": t2n(cb[2]), "cb_scores": t2n(cb[3]),
        "cos_dists": t2n(cos_d), "cos_ids": t2n(cos_i).astype(np.int64), "projected": t2n(projected),
        "template_ids": np.array([int(cc["template_id"]) for cc in corresp], np.int64),
        "template_scores": np.array([float(cc["template_score"]) for cc in corresp], np.float32),
        "cam0_f": np.asarray(loaded.template_cameras_cam_from_model[3].f, np.float64), "cam0_T": np.asarray(loaded.template_cameras_cam_from_model[3].T_world_from_eye, np.float64),
    }
    for i, cc in enumerate(corresp):
        out[f"coord_2d_ids_{i}"] = t2n(cc["coord_2d_ids"]).astype(np.int64)
        out[f"nn_vertex_ids_{i}"] = t2n(cc["nn_vertex_ids"]).astype(np.int64)
        out[f"coord_3d_{i}"] = t2n(cc["coord_3d"]).astype(np.float32)
        out[f"coord_conf_{i}"] = t2n(cc["coord_conf"]).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "wrappers.npz"), **out)
    print("wrappers.npz templates", out["template_ids"], "repre.pth bytes", os.path.getsize(os.path.join(rdir, "repre.pth")))


REPRE_IO_SCALES = [[448.0, 224.0, 112.0, 56.0]]   # extra, non-tensor entry of the file written here: the reference's loader must skip it


def gen_repre_io(ref):
    """The way back for row R: a `repre.pth` written by THIS project's save_object_repre (the representation of tests/golden/repre_ref
    plus the non-tensor extra entry) and read by the reference's own load_object_repre.  Records what that loader accepted and returned,
    so that tests/test_repre_io.py holds every later file to it without the reference: its field names (a tensor entry it does not know
    makes its constructor raise), the option-tuple fields, the top-level / projector / camera entries of the file it read, and its values
    (option dicts, camera count, the PCA projection of seeded inputs through the sklearn model it rebuilt from our tensordict)."""
    import dataclasses
    import json
    import tempfile

    from foundpose_amd import repre_util
    ours = repre_util.load_object_repre(os.path.join(OUT, "repre_ref"))
    ours.extractor_fp8_act_scales = REPRE_IO_SCALES
    with tempfile.TemporaryDirectory() as tmp:
        repre_util.save_object_repre(ours, tmp)
        written = torch.load(os.path.join(tmp, "repre.pth"), weights_only=True)
        theirs = ref.repre_util.load_object_repre(tmp, tensor_device="cpu")
    tensor_names = sorted(k for k, v in written.items() if torch.is_tensor(v))
    for name in tensor_names:
        assert torch.equal(getattr(theirs, name), getattr(ours, name)), name
    x = torch.randn(7, WRAP["raw"], generator=torch.Generator().manual_seed(1))
    proj = ref.projector_util.project_features(x, theirs.feat_raw_projectors)
    cams = theirs.template_cameras_cam_from_model
    out = {
        "repre_fields": np.array(sorted(f.name for f in dataclasses.fields(ref.repre_util.FeatureBasedObjectRepre))),
        "feat_opts_fields": np.array(ref.repre_util.FeatureOpts._fields),
        "template_desc_opts_fields": np.array(ref.repre_util.TemplateDescOpts._fields),
        "tensor_names": np.array(tensor_names),
        "other_entries": np.array(sorted(k for k, v in written.items() if not torch.is_tensor(v))),
        "projector_keys": np.array(sorted(written["feat_raw_projectors"][0]["pca_projector"])),
        "camera_keys": np.array(sorted(written["template_cameras_cam_from_model"][0])),
        "feat_opts": np.array(json.dumps(theirs.feat_opts._asdict())),
        "template_desc_opts": np.array(json.dumps(theirs.template_desc_opts._asdict())),
        "num_projectors": np.array(len(theirs.feat_raw_projectors)),
        "num_cameras": np.array(len(cams)),
        "camera_sizes": np.array([[c.width, c.height] for c in cams], np.int64),
        "proj_x": t2n(x), "proj_out": t2n(proj).astype(np.float32),
    }
    np.savez_compressed(os.path.join(OUT, "repre_io.npz"), **out)
    print("repre_io.npz tensors", tensor_names, "entries", out["other_entries"].tolist())


# ------------------------------------------------------------------ result formats
def gen_wrappers_cosine(ref):
    """`tfidf_knn_metric = "cosine"` for the visual-word search (scripts/infer.py:218-222 -> knn_util.py:52-57, 91-100): the reference's
    find_nearest_object_features / calc_tfidf / tfidf_matching / establish_correspondences over a cosine word index, on the representation
    of gen_wrappers (read back from tests/golden/repre_ref by the reference's loader).  The bank side of the descriptors is always built
    with "l2" (template_util.py:105), so the same repre.pth serves."""
    c = WRAP
    _, _, pts, feats, _, _ = build_wrapper_inputs()
    loaded = ref.repre_util.load_object_repre(os.path.join(OUT, "repre_ref"), tensor_device="cpu")
    vw = ref.knn_util.KNN(k=3, metric="cosine")
    vw.fit(loaded.feat_cluster_centroids)
    word_ids, word_dists = ref.template_util.find_nearest_object_features(query_features=feats, knn_index=vw)
    tfidf_hard = ref.template_util.calc_tfidf(word_ids, word_dists, loaded.feat_cluster_idfs, soft_assignment=False, soft_sigma_squared=10.0)
    tfidf_soft = ref.template_util.calc_tfidf(word_ids, word_dists, loaded.feat_cluster_idfs, soft_assignment=True, soft_sigma_squared=10.0)
    tm_ids, tm_scores = ref.template_util.tfidf_matching(feats, loaded, 5, vw)
    tpl_idx = []
    for t in range(c["T"]):
        idx = ref.knn_util.KNN(k=1, metric="l2")
        idx.fit(loaded.feat_vectors[torch.nonzero(loaded.feat_to_template_ids == t).flatten()])
        tpl_idx.append(idx)
    corresp = ref.corresp_util.establish_correspondences(
        query_points=pts, query_features=feats, object_repre=loaded, template_matching_type="tfidf", feat_matching_type="cyclic_buddies",
        top_n_templates=5, top_k_buddies=300, visual_words_knn_index=vw, template_knn_indices=tpl_idx, debug=True)
    l2 = ref.knn_util.KNN(k=3, metric="l2")
    l2.fit(loaded.feat_cluster_centroids)
    l2_ids = ref.template_util.find_nearest_object_features(query_features=feats, knn_index=l2)[0]
    out = {"word_ids": t2n(word_ids).astype(np.int64), "word_dists": t2n(word_dists), "tfidf_hard": t2n(tfidf_hard), "tfidf_soft": t2n(tfidf_soft),
           "tm_ids": t2n(tm_ids).astype(np.int64), "tm_scores": t2n(tm_scores), "l2_word_ids": t2n(l2_ids).astype(np.int64),
           "template_ids": np.array([int(x["template_id"]) for x in corresp], np.int64),
           "template_scores": np.array([float(x["template_score"]) for x in corresp], np.float32)}
    for i, x in enumerate(corresp):
        out[f"coord_2d_ids_{i}"] = t2n(x["coord_2d_ids"]).astype(np.int64)
        out[f"nn_vertex_ids_{i}"] = t2n(x["nn_vertex_ids"]).astype(np.int64)
    np.savez_compressed(os.path.join(OUT, "wrappers_cosine.npz"), **out)
    print("wrappers_cosine.npz templates", out["tm_ids"], "word rows differing from l2:", int((out["word_ids"] != out["l2_word_ids"]).any(1).sum()), "of", len(out["word_ids"]))


def results_inputs():
    """Seeded stand-ins for what the driver hands the evaluator: per object a few instances, each with a pose in the crop camera's
    world, the original and the crop camera, the per-stage times and a correspondence set (with repeated query ids: the score is
    the many-to-many aware inlier ratio)."""
    rng = np.random.default_rng(42)
    out = []
    for lid, n_inst in ((1, 3), (2, 2)):
        verts = rng.normal(0, 40.0, (500, 3))
        for j in range(n_inst):
            ang = rng.normal(0, 1.0, 3)
            th = np.linalg.norm(ang)
            k = ang / th
            Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
            t = np.array([rng.normal(0, 20), rng.normal(0, 20), 900 + 100 * rng.random()])
            T_oc = np.eye(4)
            T_oc[:3, 3] = [5.0 * j, -3.0, 1.0]                       # the original camera sits off the world origin
            a = 0.05 * (j + 1)
            T_cc = np.eye(4)
            T_cc[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])   # the crop camera looks at the object
            n_c = 60
            vid = rng.integers(0, 500, n_c)
            qid = rng.integers(0, 25, n_c)                            # repeated query ids
            f, c = (700.0, 705.0), (210.0, 208.0)
            Tm2c = np.linalg.inv(T_cc) @ np.block([[R, t[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]])
            pc = verts[vid] @ Tm2c[:3, :3].T + Tm2c[:3, 3]
            uv = np.stack([f[0] * pc[:, 0] / pc[:, 2] + c[0], f[1] * pc[:, 1] / pc[:, 2] + c[1]], 1)
            uv[::3] += rng.normal(0, 30.0, uv[::3].shape)              # a third of the matches are outliers
            times = {k_: float(v) for k_, v in zip(("prep", "feat_extract", "grid_sample", "proj", "corresp", "pose_coarse", "final_select"),
                                                   rng.random(7) * 0.05)}
            out.append(dict(lid=lid, scene_id=3 + lid, im_id=10 * j + 1, inst_id=j, verts=verts, R=R, t=t, T_oc=T_oc, T_cc=T_cc, f=f, c=c,
                            nn_vertex_ids=vid, coord_2d=uv, coord_2d_ids=qid, times=times, cnos_time=0.125 * (j + 1)))
    return out


def gen_results(ref):
    """estimated-poses.json through the reference's EvaluatorPose.update_without_anno / save_results_json (utils/eval_util.py:231-355)
    and the BOP19 csv through the reference's scripts/prepare_bop_submission.py run on those files; the fixture keeps both outputs."""
    import importlib
    import runpy
    import shutil
    import tempfile
    import types as _types
    bop = _types.ModuleType("bop_toolkit_lib")
    tmp = tempfile.mkdtemp()
    for sub in ("inout", "config", "dataset_params", "misc", "renderer", "visibility", "pose_error"):
        m = _types.ModuleType(f"bop_toolkit_lib.{sub}")
        setattr(bop, sub, m)
        sys.modules[f"bop_toolkit_lib.{sub}"] = m
    sys.modules["bop_toolkit_lib"] = bop
    for name, attrs in (("skimage", ()), ("skimage.color", ("label2rgb",)), ("skimage.feature", ("canny",)), ("skimage.morphology", ("binary_dilation",)),
                        ("imageio", ()), ("trimesh", ()), ("pyrender", ()), ("distinctipy", ())):   # visualisation-only imports of html_util / eval_errors
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = _types.ModuleType(name)
                for a_ in attrs:
                    setattr(m, a_, None)
                sys.modules[name] = m
    bop.config.output_path, bop.config.datasets_path = tmp, tmp
    bop.dataset_params.get_model_params = lambda datasets_path, dataset_name: {"obj_ids": [1, 2]}
    eu = importlib.import_module("utils.eval_util")
    structs = importlib.import_module("utils.structs")
    out_dir = os.path.join(tmp, "inference", "lmo_v1")
    dst = os.path.join(OUT, "results_ref")
    shutil.rmtree(dst, ignore_errors=True)
    for lid in (1, 2):
        ev = eu.EvaluatorPose([lid])
        for d in results_inputs():
            if d["lid"] != lid:
                continue
            mk = lambda T: structs.PinholePlaneCameraModel(width=420, height=420, f=d["f"], c=d["c"], T_world_from_eye=T)
            ev.detection_times[(d["scene_id"], d["im_id"])] = d["cnos_time"]
            ev.update_without_anno(scene_id=d["scene_id"], im_id=d["im_id"], inst_id=d["inst_id"], hypothesis_id=0, object_repre_vertices=d["verts"],
                                   obj_lid=lid, object_pose_m2w=structs.ObjectPose(R=d["R"], t=d["t"].reshape(3, 1)), orig_camera_c2w=mk(d["T_oc"]),
                                   camera_c2w=mk(d["T_cc"]), time_per_inst=d["times"],
                                   corresp={"nn_vertex_ids": d["nn_vertex_ids"], "coord_2d": d["coord_2d"], "coord_2d_ids": d["coord_2d_ids"]}, inlier_radius=10)
        os.makedirs(os.path.join(out_dir, str(lid)), exist_ok=True)
        ev.save_results_json(os.path.join(out_dir, str(lid), "estimated-poses.json"))
        os.makedirs(os.path.join(dst, str(lid)), exist_ok=True)
        shutil.copy(os.path.join(out_dir, str(lid), "estimated-poses.json"), os.path.join(dst, str(lid), "estimated-poses.json"))
    runpy.run_path(os.path.join(ref_shim.REF_ROOT, "scripts", "prepare_bop_submission.py"), run_name="__main__")
    shutil.copy(os.path.join(out_dir, "coarse_lmo-estimated-poses.csv"), os.path.join(dst, "coarse_lmo-estimated-poses.csv"))
    shutil.rmtree(tmp, ignore_errors=True)
    print("results_ref", sorted(os.listdir(dst)), open(os.path.join(dst, "coarse_lmo-estimated-poses.csv")).read().count("\n") + 1, "csv lines")


def main():
    if not ref_shim.reference_available():
        sys.exit("reference not present; fixtures can only be generated in the build container")
    os.makedirs(OUT, exist_ok=True)
    ref = ref_shim.import_reference()
    gen_match(ref)
    gen_points(ref)
    gen_extractor(ref)
    gen_extractor_420(ref)
    gen_extractor_stride(ref)
    gen_extractor_noreg(ref)
    gen_hot_section(ref)
    gen_crop(ref)
    gen_lift(ref)
    gen_wrappers(ref)
    gen_repre_io(ref)
    gen_wrappers_cosine(ref)
    gen_results(ref)


if __name__ == "__main__":
    if len(sys.argv) > 1:  # python -m oracle.make_golden gen_extractor_420 ... : regenerate single fixtures
        if not ref_shim.reference_available():
            sys.exit("reference not present; fixtures can only be generated in the build container")
        os.makedirs(OUT, exist_ok=True)
        _ref = ref_shim.import_reference()
        for _name in sys.argv[1:]:
            globals()[_name](_ref)
    else:
        main()
