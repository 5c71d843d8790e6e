#!/usr/bin/env python3
"""Maps the chunk latents of a trained chunk autoencoder into the plane on the MI355X kernels (gesture2vec_amd/embedding.py): the
reference's `PCA(50)` + `TSNE(2, perplexity=30)` picture of all latents coloured by code (`Clustering.py:1046-1056`, `:1411-1417`).

    python embed_latents.py --checkpoint ckpt.bin --chunks x.npy [--kmeans model.pk] [--sample-rows M] [--out map.npz]
                            [--scatter-txt scatter.txt] [--place-rest] [--save-map map.pk] [--map map.pk] [--quality K]

`--chunks` holds (N, T, D) pose chunks in the autoencoder's input space.  Their latents and code ids (`chunks_to_codes`; for an
autoencoder without a quantiser the ids of the pickled `--kmeans` model, or none) are taken on the device, `--sample-rows M` rows are
drawn as sklearn's `sample_size` (seeded with `--seed`; needed beyond `ops.tsne_max_rows()` rows) and mapped with `latent_map`.
`--out` (default `<checkpoint dir>/plots/latent_map.npz`) receives `coords` (M, 2) fp32, `codes` (M,) int64 (-1 without ids) and
`rows` (M,) int64, the mapped rows of `--chunks`.  `--scatter-txt` also writes the text of the reference's `make_unity_scatter`
(`Clustering.py:1339-1345`): a first line "512", then `<code>,<x>,<y>` with three decimals per row.  No plot is drawn.

With `--sample-rows M --place-rest` every row of `--chunks` is mapped, however many there are: the sample exactly, each other row
placed into the sample's map (`LatentMap.fit_all`); `coords`, `codes` and `rows` then cover all rows in input order and `fitted` (N,)
bool marks the sample.  `--save-map PATH` pickles the fitted `LatentMap`.  `--map PATH` fits nothing: the rows of `--chunks` (a
generated set, say) are placed into that saved map, which is how the reference's `Metrics_analysis` draws a generated sequence as a
trajectory through the map of the real data (`Clustering.py:1318-1350`).

`--quality K` says how far the map can be believed: trustworthiness and continuity over K neighbours (`embedding.map_quality`,
sklearn's definition, between the PCA scores the map was made from and the map) are printed, and each row's share of the two
penalty sums goes to the `.npz` as `penalty_t` and `penalty_c` (int64, in the order of `rows`), so that badly mapped rows can be
found.  With `--place-rest` the two numbers are printed separately for the sample and for the placed rows, the latter scored
against the sample (`embedding.placement_quality`); with `--map`, for the placed rows against the saved map's own rows."""
from __future__ import annotations

import argparse
import os
import pickle
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from utils.train_utils import load_checkpoint_and_model  # noqa: E402
from gesture2vec_amd.embedding import LatentMap, latent_map, placement_quality  # noqa: E402
from gesture2vec_amd.pipeline import chunk_latents, chunks_to_codes  # noqa: E402


def scatter_text(codes, coords) -> str:
    """the reference's make_unity_scatter text"""
    return "512\n" + "".join("{},{:.3f},{:.3f}\n".format(int(c), float(x), float(y)) for c, (x, y) in zip(codes, coords))


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", required=True, help="chunk autoencoder checkpoint (train_autoencoder_VQVAE.py)")
    ap.add_argument("--chunks", required=True, help=".npy of (N, T, D) pose chunks")
    ap.add_argument("--kmeans", default=None, help="pickled gesture2vec_amd.kmeans.KMeans: the code ids of a quantiser-free autoencoder")
    ap.add_argument("--sample-rows", dest="sample_rows", type=int, default=None, help="map this many rows, drawn as sklearn's sample_size")
    ap.add_argument("--n-pca", dest="n_pca", type=int, default=50)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--max-iter", dest="max_iter", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="map path (default: <checkpoint dir>/plots/latent_map.npz)")
    ap.add_argument("--scatter-txt", dest="scatter_txt", default=None, help="also write the reference's make_unity_scatter text here")
    ap.add_argument("--place-rest", dest="place_rest", action="store_true",
                    help="with --sample-rows: place every other row into the sample's map and write all rows")
    ap.add_argument("--save-map", dest="save_map", default=None, help="pickle the fitted LatentMap here")
    ap.add_argument("--map", dest="map", default=None, help="a pickled LatentMap: fit nothing, place the rows of --chunks into it")
    ap.add_argument("--quality", type=int, default=None, metavar="K",
                    help="print trustworthiness and continuity over K neighbours and write each row's penalties")
    ap.add_argument("--batch_rows", type=int, default=65536)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.place_rest and a.sample_rows is None:
        ap.error("--place-rest needs --sample-rows")
    if a.map and (a.place_rest or a.save_map or a.sample_rows is not None):
        ap.error("--map places into a saved map: it goes with neither --sample-rows, --place-rest nor --save-map")
    dev = torch.device(a.device)
    _, net, _, _, _ = load_checkpoint_and_model(a.checkpoint, dev, "autoencoder_vq")
    net.eval()
    chunks = torch.from_numpy(np.load(a.chunks).astype(np.float32, copy=False)).to(dev)
    km = None
    if a.kmeans:
        with open(a.kmeans, "rb") as f:
            km = pickle.load(f)
    lats, ids = [], []
    for s in range(0, chunks.shape[0], a.batch_rows):
        if getattr(net, "vq", True) or km is not None:
            lat, idx = chunks_to_codes(net, chunks[s:s + a.batch_rows], kmeans=km)
        else:
            lat, idx = chunk_latents(net, chunks[s:s + a.batch_rows]), None
        lats.append(lat)
        ids.append(idx)
    lat = torch.cat(lats)
    codes = None if ids[0] is None else torch.cat(ids)
    print(f"latents: {tuple(lat.shape)}")
    fitted, quality = None, None
    if a.map:
        with open(a.map, "rb") as f:
            lm = pickle.load(f)
        coords, rows = lm.transform(lat), torch.arange(lat.shape[0], device=dev)
        if a.quality:
            quality = {"fitted": None, "placed": placement_quality(lm.tsne.fit_rows_.to(dev), lm.coords_.to(dev), lm.pca.transform(lat),
                                                                   coords, n_neighbors=a.quality)}
    elif a.place_rest or a.save_map or a.quality:
        lm = LatentMap(n_pca=a.n_pca, sample_size=a.sample_rows, random_state=a.seed, perplexity=a.perplexity, max_iter=a.max_iter)
        if a.place_rest:
            (coords, fitted), rows = lm.fit_all(lat), torch.arange(lat.shape[0], device=dev)
        else:
            lm.fit(lat)
            coords, rows = lm.coords_, lm.rows_
        if a.quality:
            quality = (lm.quality(lat, coords, n_neighbors=a.quality) if a.place_rest else
                       lm.quality(lat[rows].contiguous(), coords, sample_idx=torch.arange(rows.shape[0]), n_neighbors=a.quality))
        if a.save_map:
            with open(a.save_map, "wb") as f:
                pickle.dump(lm, f)
            print(f"wrote {a.save_map}")
    else:
        coords, rows = latent_map(lat, n_pca=a.n_pca, sample_size=a.sample_rows, random_state=a.seed, perplexity=a.perplexity,
                                  max_iter=a.max_iter)
    res = {"coords": coords.cpu().numpy(), "rows": rows.cpu().numpy(),
           "codes": np.full(rows.shape[0], -1, np.int64) if codes is None else codes[rows].cpu().numpy()}
    if fitted is not None:
        res["fitted"] = fitted.cpu().numpy()
    if quality is not None:
        res["penalty_t"], res["penalty_c"] = (np.zeros(rows.shape[0], np.int64) for _ in range(2))
        for part, name in (("fitted", "sample" if quality["placed"] is not None else "map"), ("placed", "placed rows")):
            q = quality[part]
            if q is not None:
                print(f"{name}: trustworthiness {q['trustworthiness']!r}, continuity {q['continuity']!r} over {q['n_neighbors']} "
                      f"neighbours of {q['penalty_t'].shape[0]} rows")
                at = q["rows"].cpu().numpy() if "rows" in q else slice(None)          # (LatentMap.quality names the rows of each part)
                res["penalty_t"][at] = q["penalty_t"].cpu().numpy()
                res["penalty_c"][at] = q["penalty_c"].cpu().numpy()
        res["quality"] = {part: None if q is None else (q["trustworthiness"], q["continuity"]) for part, q in quality.items()}
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.checkpoint)), "plots", "latent_map.npz")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **{name: v for name, v in res.items() if name != "quality"})
    print(f"wrote {out}: {res['coords'].shape[0]} rows")
    if a.scatter_txt:
        with open(a.scatter_txt, "w") as f:
            f.write(scatter_text(res["codes"], res["coords"]))
        print(f"wrote {a.scatter_txt}")
    return res


if __name__ == "__main__":
    main()
