"""End-to-end evaluate loop on one GPU (BASELINE.json configs[3] shape, single rank): a synthetic data set of 512x512 gray PNGs on disk,
`predict_unet_cover` (reference-faithful per-image path) vs `predict_unet_cover_batched` (u8 upload -> forward -> fused WS statistics).
Prints one JSON line.  Usage: python tools/bench_evaluate.py [--images 256] [--batch 32] [--mode bf16x3]"""
import argparse, json, sys, tempfile, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from PIL import Image
from ws_unet_amd import evaluate, fabrika, formula, planes, unet_run
from ws_unet_amd.model import get_model

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=256)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--mode", default="f16f4p")
ap.add_argument("--per-image-rows", type=int, default=256, help="rows of the per-image leg (raise it for a leg that times long enough to compare)")
a = ap.parse_args()
root = Path(tempfile.mkdtemp())
(root / "images").mkdir()
u8 = formula.synthetic_images(a.images, 512, 512, seed=99)
t0 = time.perf_counter()
for i in range(a.images):
    Image.fromarray(u8[i]).save(root / "images" / f"{i}.png", compress_level=1)
(root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{i}.png,512,512\n" for i in range(a.images)))
t_write = time.perf_counter() - t0
m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=0., mode=a.mode)
m.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()})
m = m.to("cuda")
batched = fabrika.precovers(iterator="batched", convert_to="pandas", ignore_missing=False, batch_size=a.batch)(
    fabrika.shared_kwargs(evaluate.predict_unet_batch, ("model", "imread", "device"), evaluate._prefetch_planes))
batched(root, model=m, take_num_images=a.batch)                 # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter(); dfb = batched(root, model=m); torch.cuda.synchronize(); t_b = time.perf_counter() - t0
n1 = min(a.images, a.per_image_rows)
evaluate.predict_unet_cover(root, model=m, take_num_images=8, progress_on=False)            # warm-up: range look, decode threads
t0 = time.perf_counter(); df1 = evaluate.predict_unet_cover(root, model=m, take_num_images=n1, progress_on=False); torch.cuda.synchronize(); t_1 = time.perf_counter() - t0
xd = planes.load_planes_u8([str(root / "images" / "0.png")]).to("cuda")
t0 = time.perf_counter()
for _ in range(200):
    unet_run.predict_u8_one_readback(xd, m)
t_e = (time.perf_counter() - t0) / 200
t0 = time.perf_counter()
for i in range(min(a.images, 64)):
    np.array(Image.open(root / "images" / f"{i}.png"))
t_dec = (time.perf_counter() - t0) / min(a.images, 64)            # PIL on one thread (what the reference's per-image read costs; libwsu_io: decode_ms_per_image_per_thread)
err = float(np.abs(dfb["beta_hat"].to_numpy(float)[:n1] - df1["beta_hat"].to_numpy(float)).max())
# the host budget of the file-fed pass (VERDICT r03 next #7a) and the same pass fed from pre-decoded uint8 shards (#7d)
files = [str(root / "images" / f"{i}.png") for i in range(a.images)]
x = planes.load_planes_u8(files[:a.batch]).to("cuda")
for _ in range(3):
    unet_run.predict_u8_batch(x, m)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    unet_run.predict_u8_batch(x, m)
torch.cuda.synchronize()
gpu_rate = 10 * a.batch / (time.perf_counter() - t0)             # images/s of the device side alone (planes resident)
budget = planes.decode_budget(files, gpu_images_per_s=gpu_rate, sample=32)
planes.use_u8_shards(planes.write_u8_shards(files, root / "shards"))
batched(root, model=m, take_num_images=a.batch)
torch.cuda.synchronize()
t0 = time.perf_counter(); dfs = batched(root, model=m); torch.cuda.synchronize(); t_s = time.perf_counter() - t0
planes.use_u8_shards(None)
same = bool(np.array_equal(dfs["beta_hat"].to_numpy(), dfb["beta_hat"].to_numpy()) and np.array_equal(dfs["l1"].to_numpy(), dfb["l1"].to_numpy()))
print(json.dumps({"metric": "evaluate loop images/s (PNG on disk -> beta_hat, l1)", "mode": a.mode, "images": a.images,
                  "batched_images_per_s": a.images / t_b, "per_image_api_images_per_s": n1 / t_1, "one_image_call_ms_resident_plane": t_e * 1e3,
                  "png_decode_ms_per_image_1thread_PIL": t_dec * 1e3, "max_abs_beta_diff_batched_vs_per_image": err,
                  "gpu_only_images_per_s": gpu_rate, "decode_ms_per_image_per_thread": budget["decode_ms_per_image_per_thread"],
                  "decode_threads_needed_per_rank_at_gpu_rate": budget["threads_needed_per_rank"], "usable_cores": budget["usable_cores"],
                  "decode_threads_used": budget["decode_threads_used"],
                  "batched_from_u8_shards_images_per_s": a.images / t_s, "u8_shards_table_identical": same,
                  "note": "batched path: PNG decode by libwsu_io on C++ threads, one chunk ahead of the GPU (fabrika iterator='batched' prefetch); the per-image API decodes the files of the next 48 rows on helper threads (libwsu_io); rows already decoded ride along in the launch of the row asked for (<= 16 images), two launches are queued ahead, statistics + range flag of a launch come back in one copy"}))
