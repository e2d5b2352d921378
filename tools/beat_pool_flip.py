#!/usr/bin/env python3
"""CPU experiment behind the T = 1030 cases of tests/test_gpu_beat_train.py: in the fp64 restatement of the Beat-Transformer's loss, flip the max-pool
choice of every cell whose top two candidates lie within a threshold (by nudging the runner-up past the maximum, which changes no value by more than the threshold) and
print how far the conv gradients move.  Pools: 0 = after conv1, 1 = after conv2, 2 = after conv3.  Not a test.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import beat_train_np as B
from etude_amd import synth
dims=synth.beat_dims(nlayers=9,d_hid=256); sd=synth.beat_state_dict(13,dims)
b=B.make_batch(34,(1030,))
kw=dict(pos_weight=(3.0,7.0),tempo_weight=0.5)
l,g0=B.loss_and_grads(sd,9,b,torch.float64,**kw)
orig=B._pool3
calls={'n':0}
def make(which, thresh):
    def pool(x, diag, name):
        i=calls['n']%3; calls['n']+=1
        if i==which:
            n=x.shape[-1]//3
            v=x[...,:3*n].reshape(*x.shape[:-1],n,3).detach()
            top=v.sort(-1)
            gap=top.values[...,2]-top.values[...,1]
            m=gap<thresh
            print('pool',which,'cells flipped',int(m.sum()),'of',m.numel())
            # add 2*gap at runner-up position
            ru=top.indices[...,1]
            d=torch.zeros_like(v); d.scatter_(-1, ru[...,None], (2*gap*m)[...,None])
            pad=torch.zeros_like(x); pad[...,:3*n]=d.reshape(*x.shape[:-1],3*n)
            x=x+pad
        return orig(x,diag,name)
    return pool
for which,th in ((0,1e-7),(1,2e-7),(2,1e-7),(0,1e-6),(1,1e-6),(2,1e-6)):
    calls['n']=0
    B._pool3=make(which,th)
    l2,g=B.loss_and_grads(sd,9,b,torch.float64,**kw)
    print(which,th,{k:'%.2e'%B.rel_err(g[k],g0[k]) for k in ['conv1.weight','conv1.bias','conv2.weight','conv2.bias','conv3.weight','conv3.bias']})
B._pool3=orig
