"""Weight-quantization report of a model: per quantized weight its width, channel count, SQNR on the training grid and the share of
channels whose range is narrower than their observed min/max (qat_utils.weight_quant_report).

  python tools/wq_report.py -y configs/convtasnet_2spks_8k_synthetic_w4_mse.yaml [--ckpt best_model.pth] [--use_cpu]

Without --ckpt the model is built as the trainer builds it and every weight quantizer observes its weight once with the configured
`weight_observer` (minmax | mse): the ranges training would start from.  With --ckpt the stored ranges are reported."""
import argparse
import os
import sys

import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import _lib  # noqa: E402
from fqss_amd.quantization.qat.models.load_model import create_model, load_checkpoint, quantize_model  # noqa: E402
from fqss_amd.quantization.qat.qat_utils import weight_quant_report, weight_quantizer_pairs  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--yml_path", "-y", required=True, help="YML configuration file")
    p.add_argument("--ckpt", default=None, help="state_dict of the quantized model (best_model.pth)")
    p.add_argument("--use_cpu", action="store_true", help="CPU backend")
    args = p.parse_args()
    conf = yaml.safe_load(open(args.yml_path))
    if args.use_cpu:
        _lib.set_backend("cpu")
    device = "cpu" if args.use_cpu else "cuda"
    model = quantize_model(create_model(conf["model_cfg"]), conf["model_cfg"]["quantization"])
    if args.ckpt:
        sd = load_checkpoint(args.ckpt)
        for key in ("state", "state_dict"):
            if key in sd:
                sd = sd[key]
                break
        model.load_state_dict(sd, strict=True)
    model = model.to(device)
    if not args.ckpt:
        with torch.no_grad():
            for wqm, w, _ in weight_quantizer_pairs(model):
                if wqm.observer_mode:
                    wqm(w)              # the observer call: writes the ranges, returns the weight unchanged
    rows = weight_quant_report(model)
    observer = conf["model_cfg"]["quantization"].get("weight_observer", "minmax")
    print(f"# {args.yml_path}: {len(rows)} quantized weights, " + (f"ranges of {args.ckpt}" if args.ckpt else f"weight_observer {observer}"))
    print(f"{'parameter':64s} {'bits':>4s} {'chan':>5s} {'SQNR dB':>8s} {'narrower':>8s}")
    for r in rows:
        print(f"{r['name']:64s} {r['n_bits']:4d} {r['channels']:5d} {r['sqnr_db']:8.2f} {100.0 * r['narrower']:7.1f}%")


if __name__ == "__main__":
    main()
