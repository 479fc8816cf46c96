"""Bit comparison of two library builds on the deterministic backward: in deterministic mode gacc_add sums in fixed point, so a parameter
gradient depends only on each workgroup's partial sums, not on the order they arrive in.  Two builds whose kernels keep their grids and
their summation order inside a workgroup give bit-identical gradients.

    python tools/wgrad_bits.py LIB_A LIB_B        # "cur" = the default library

One fresh child process per library (OFD_LIB selects it) runs one deterministic training step per model and saves every parameter
gradient: the models and sizes of test_unet_backward_deterministic_mode_is_bit_reproducible, (2, 32, 48) and (3, 24, 104), and the
wide-input model of test_wide_input_deterministic_mode_is_bit_reproducible (the 7x7 weight gradient of a 48-channel packing).  Exit
status 0: every gradient torch.equal between the two, no accumulation missed its shadow under either."""
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(path):
    import torch
    from opticalflowdiffusion_amd import Unet
    from opticalflowdiffusion_amd.warp import nan_mse
    out = {}

    def run(tag, net, x, cond, t, target):
        net.set_deterministic(True)
        loss = nan_mse(net(x.cuda(), external_cond=cond.cuda(), time=t.cuda()), target.cuda())
        loss.backward()
        torch.cuda.synchronize()
        out[tag + "/misses"] = torch.tensor(net.deterministic_misses())
        out[tag + "/loss"] = loss.detach().cpu()
        for n, p in net.named_parameters():
            out[tag + "/" + n] = p.grad.detach().cpu()

    for B, H, W in ((2, 32, 48), (3, 24, 104)):
        torch.manual_seed(11)
        net = Unet(64, channels=5, out_dim=2).cuda()
        run(f"unet{B}x{H}x{W}", net, torch.randn(B, 2, H, W), torch.rand(B, 3, H, W) * 2 - 1, torch.tensor([17, 803, 400][:B]), torch.randn(B, 2, H, W))
    torch.manual_seed(21)
    net = Unet(64, channels=35, out_dim=2).cuda()
    B, H, W = 2, 32, 48
    run("wide35", net, torch.randn(B, 18, H, W), torch.rand(B, 17, H, W) * 2 - 1, torch.tensor([3, 900]), torch.randn(B, 2, H, W))
    torch.save(out, path)


def main():
    if sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    import torch
    dumps = []
    with tempfile.TemporaryDirectory() as d:
        for i, lib in enumerate(sys.argv[1:3]):
            env = dict(os.environ)
            env.pop("OFD_LIB", None)
            if lib != "cur":
                env["OFD_LIB"] = os.path.abspath(lib)
            path = os.path.join(d, f"grads{i}.pt")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], env=env, check=True)
            dumps.append(torch.load(path))
    a, b = dumps
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    missed = {k: (int(a[k]), int(b[k])) for k in a if k.endswith("/misses") and (int(a[k]) or int(b[k]))}
    print(f"{len(a)} tensors compared ({sum(v.numel() for v in a.values())} elements): {len(bad)} differ; deterministic misses: {missed or 0}")
    for k in bad:
        print(f"  {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} elements, max |diff| {float((a[k] - b[k]).abs().max()):.3e}")
    sys.exit(1 if bad or missed else 0)


if __name__ == "__main__":
    main()
