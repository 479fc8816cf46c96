#!/bin/bash
# same-box per-layer A/B of library builds, alternating: tools/ab_conv_shapes.sh rounds tag1 tag2 ...  ("cur" = the default library);
# other arguments of tools/conv_shape_ab.py through CONV_SHAPE_ARGS.  Stops at the first run that fails.
R=$1; shift
for r in $(seq $R); do for v in "$@"; do if [ $v = cur ]; then unset OFD_LIB; else export OFD_LIB=$PWD/opticalflowdiffusion_amd/lib/libofd_hip_$v.so; fi
timeout -k 10 120 python tools/conv_shape_ab.py --tag $v $CONV_SHAPE_ARGS || exit 1; done; done
