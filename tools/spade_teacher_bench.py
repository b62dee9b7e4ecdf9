"""Step time and library-call count of the GauGAN teacher step (`--model spade`, cat_amd/models/spade_model.py), with the discriminator's
loss head as one MultiLossFn call each way (default) and as one LossFn per term (CAT_LOSS_MULTI=0).

Synthetic 512 x 256 input (crop 512, aspect 2), batch 4, 35 labels + edges, ngf 64, ndf 64, num_D 2, n_layers_D 4, hinge + feature matching +
VGG (full width, torch's default initialisation: timing does not depend on the values), TTUR.  Per run: 5 warm-up steps, then HIP events
around 10 steps on the stream (one synchronisation at the end); afterwards 2 more steps under the library's profiling hook, which counts the
entry-point calls of libcat_hip per kernel family (a `loss` call is 2 launches forward or 1 backward; a `loss_multi` call likewise, for up to
16 terms).  The switch is read once at import, so every run is a child process; the two modes alternate over --repeats runs each.

    python tools/spade_teacher_bench.py [--repeats 3] [--steps 10] [--warmup 5]         # prints a table and one JSON line"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, BATCH = 256, 512, 4


def child(a):
    import ctypes as C

    import torch
    from cat_amd import _lib, spade_model_modules, synthetic
    from cat_amd.models import create_model
    opt = synthetic.default_options(norm='instance', gpu_ids=[0])
    opt.__dict__.update(dict(
        model='spade', input_nc=35, output_nc=3, semantic_nc=36, contain_dontcare_label=False, no_instance=False, ngf=64, netG='inception_spade',
        norm_G='spadesyncbatch3x3', num_upsampling_layers='more', crop_size=W, aspect_ratio=2.0, dropout_rate=0, netD='multi_scale', ndf=64,
        n_layers_D=4, num_D=2, norm_D='spectralinstance', init_type='xavier', init_gain=0.02, active_fn='nn.LeakyReLU', gan_mode='hinge',
        lambda_gan=1.0, lambda_feat=10.0, lambda_vgg=10.0, no_TTUR=False, lr=2e-4, beta1=0.5, beta2=0.999, no_fid=True, no_mIoU=True,
        restore_G_path=None, restore_D_path=None, restore_O_path=None))
    torch.manual_seed(233)
    model = create_model(opt, verbose=False)
    model.modules_on_one_gpu.train()
    batches = []
    for i in range(2):
        lab, ins = synthetic.label_maps(BATCH, H, W, 3000 + 10 * i)
        batches.append({'label': lab.cuda(), 'instance': ins.cuda(), 'image': synthetic.images((BATCH, 3, H, W), 4000 + 10 * i).cuda(), 'path': []})

    def step(i):
        model.set_input(batches[i % 2])
        model.optimize_parameters(i)

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(a.steps):
        step(a.warmup + i)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    lib = _lib.load()
    nprof = 2
    lib.cat_prof_enable(1)
    for i in range(nprof):
        step(i)
    torch.cuda.synchronize()
    n = lib.cat_prof_collect()
    lib.cat_prof_enable(0)
    fams, name = {}, C.create_string_buffer(64)
    cnt, tms, fl = C.c_int64(), C.c_double(), C.c_double()
    for i in range(n):
        lib.cat_prof_family(i, name, 64, C.byref(cnt), C.byref(tms), C.byref(fl))
        fams[name.value.decode()] = cnt.value / nprof
    losses = {k: float(v) for k, v in model.get_current_losses().items()}
    print('RESULT ' + json.dumps(dict(loss_multi=spade_model_modules.loss_multi_enabled(), ms_per_step=ms, images_per_s=BATCH / ms * 1e3,
                                      calls_per_step=sum(fams.values()), loss_calls=fams.get('loss', 0.0), loss_multi_calls=fams.get('loss_multi', 0.0),
                                      finite=all(v == v and abs(v) < 1e30 for v in losses.values()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {'1': [], '0': []}
    for _ in range(a.repeats):
        for mode in ('1', '0'):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--steps', str(a.steps), '--warmup', str(a.warmup)]
            p = subprocess.run(cmd, env=dict(os.environ, CAT_LOSS_MULTI=mode), capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
            if p.returncode != 0 or not line:
                sys.exit('child run failed (CAT_LOSS_MULTI=%s, exit %d):\n%s' % (mode, p.returncode, (p.stdout + p.stderr)[-3000:]))
            runs[mode].append(json.loads(line[0][7:]))
    print('GauGAN teacher step, %d x %d, batch %d, ngf 64, ndf 64: %d warm-up + %d timed steps per run' % (W, H, BATCH, a.warmup, a.steps))
    print('loss head       ms/step (runs)                  images/s   library calls/step   loss calls   loss_multi calls')
    for mode, label in (('1', 'MultiLossFn'), ('0', 'per-term LossFn')):
        r = runs[mode]
        ms = sorted(x['ms_per_step'] for x in r)
        med = ms[len(ms) // 2]
        print('%-15s %8.2f (%s)   %8.1f   %18.1f   %10.1f   %16.1f' % (label, med, ' '.join('%.2f' % v for v in ms), BATCH / med * 1e3,
                                                                      r[0]['calls_per_step'], r[0]['loss_calls'], r[0]['loss_multi_calls']))
    print(json.dumps(dict(tool='spade_teacher_bench', image=[H, W], batch=BATCH, steps=a.steps, warmup=a.warmup, multi=runs['1'], per_term=runs['0'])))


if __name__ == '__main__':
    main()
