"""Slide-level zero-shot by top-K pooling: ``PLIP.slide_zero_shot`` on synthetic slides.

    python examples/slide_zero_shot.py

Every tile of a slide is scored against every class prototype; for each class the K largest tile scores are averaged, and the slide takes
the class of the largest pooled score (MI-Zero, CONCH).  K is the knob: K = 1 asks "is there ONE tile that looks like the class", a large
K asks "does a good part of the slide look like it".  The slides below are built from two tile populations so that the two questions have
different answers: mostly "stroma"-like tiles with a few strongly "tumor"-like ones.  A real caller passes the embeddings
``encode_images`` / ``encode_region`` returned and a real checkpoint (``PLIP("path/to/plip")``); weights and tiles here are synthetic,
and the prompts are token ids because no vocabulary is on disk.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from plip_amd import weights as W
    from plip_amd.bags import bag_mean, bag_offsets, class_prototypes
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    from plip_amd.plip import PLIP
    cfg = get_config("ViT-B/32")
    plip = PLIP(model=PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=256))
    # two prompts as token ids ("<bos> w1 w2 <eos>"), one prototype per class -- with a tokenizer: plip.class_prototypes([["tumor"], ["stroma"]])
    ids = np.full((2, cfg.context_length), cfg.eos_token_id, np.int64)
    ids[0, :3], ids[1, :3] = (cfg.bos_token_id, 101, 202), (cfg.bos_token_id, 303, 404)
    protos = class_prototypes(plip.encode_text(ids, batch_size=2), [[0], [1]])
    names = ["tumor", "stroma"]
    # tile populations: `lean` along the part of one prototype that the other does not share, a little of both parts at random, and
    # noise of norm 0.3 outside the prototypes' plane (synthetic prototypes are nearly parallel: only what tells them apart is used)
    rng = np.random.default_rng(0)
    P = protos.shape[1]
    p = protos.astype(np.float64)
    rho = p[0] @ p[1]
    own = np.stack([(p[0] - rho * p[1]), (p[1] - rho * p[0])]) / np.sqrt(1 - rho * rho)      # own[c] . p[1 - c] == 0

    def tiles(n, cls, lean):
        coef = 0.03 * rng.standard_normal((n, 2))
        coef[:, cls] += lean
        g = rng.standard_normal((n, P))
        g -= np.outer(g @ p[0], p[0])
        g -= np.outer(g @ own[1], own[1])              # (p[0], own[1]) is an orthonormal basis of the plane
        g *= 0.3 / np.linalg.norm(g, axis=1, keepdims=True)
        return (coef @ own + g).astype(np.float32)
    slides = {"mostly stroma, a small tumor focus": np.concatenate([tiles(400, 1, 0.15), tiles(6, 0, 1.0)]),
              "stroma only": tiles(300, 1, 0.15),
              "tumor throughout": np.concatenate([tiles(250, 0, 0.4), tiles(50, 1, 0.15)])}
    ks = (1, 5, 10, 50, 100)
    out = plip.slide_zero_shot(list(slides.values()), protos, ks=ks, return_top_tiles=3)
    print(f"pooled scores (scale exp(logit_scale) = {np.exp(float(plip.model.logit_scale)):.1f}); rows: slides, columns: k = {ks}")
    for s, name in enumerate(slides):
        print(f"  {name} ({len(slides[name])} tiles)")
        for c, cname in enumerate(names):
            print(f"    {cname:7s}" + " ".join(f"{v:8.3f}" for v in out["pooled"][s, :, c]) + f"   best tiles {out['top_tiles'][s, c].tolist()}")
        print("    pred   " + " ".join(f"{names[p]:>8s}" for p in out["pred"][s]))
    first = out["pred"][0]
    print(f"slide 0 at k = 1: {names[first[0]]}; at k = 100: {names[first[-1]]}"
          + ("  (the focus decides a max, the bulk decides a mean)" if first[0] != first[-1] else ""))
    # the other standard slide representation: the L2-normalised mean tile embedding, one call for the cohort
    emb = np.concatenate(list(slides.values()))
    offsets, _ = bag_offsets(sizes=[len(v) for v in slides.values()])
    mean = bag_mean(plip.model.engine, emb, offsets, normalize=True)
    print("cosine of the mean tile embedding with the prototypes:")
    for s, name in enumerate(slides):
        print(f"  {name}: " + ", ".join(f"{n} {float(v):+.3f}" for n, v in zip(names, mean[s].cpu().numpy() @ protos.T)))


if __name__ == "__main__":
    main()
