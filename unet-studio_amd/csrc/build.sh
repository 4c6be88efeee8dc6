#!/bin/bash
# Builds libunet_hip.so for gfx950 in-tree (next to the Python package).  No GPU needed: hipcc cross-compiles.
# Objects are compiled in parallel (one hipcc per source) and only when the source or a header is newer.
set -e
cd "$(dirname "$0")"
SRCS="graph.cpp engine.cpp comm.cpp kernels_direct.hip kernels_elem.hip kernels_sgd_pack.hip kernels_mfma_conv.hip kernels_mfma_deep.hip kernels_mfma_conv_z16.hip kernels_mfma_s2.hip kernels_mfma_s2_wgrad.hip kernels_mfma_wgrad.hip kernels_mfma_wgrad_z.hip kernels_mfma_wgrad_zd.hip kernels_augment.hip kernels_mfma_f32.hip kernels_qc.hip kernels_feed.hip kernels_postproc.hip kernels_space.hip kernels_tiles.hip kernels_mirror.hip kernels_ensemble.hip kernels_preproc.hip kernels_components.hip kernels_atlas.hip kernels_register.hip kernels_table.hip kernels_distance.hip kernels_instances.hip kernels_morph.hip kernels_stats.hip kernels_calib.hip kernels_recal.hip kernels_patches.hip kernels_coreg.hip kernels_start.hip kernels_warp.hip kernels_cowarp.hip kernels_deform.hip kernels_bias.hip"
FLAGS="-O3 --offload-arch=gfx950 -fPIC -std=c++17 -Wno-unused-result"
mkdir -p build
newest_hdr=$(ls -t *.h *.hpp ../../include/*.h | head -1)
todo=""
for f in $SRCS; do
    o=build/${f%.*}.o
    if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ "$newest_hdr" -nt "$o" ]; then todo="$todo $f"; fi
done
[ -f ../asm_loads_check_conv_z.json ] || todo="$todo check:kernels_mfma_conv.hip"
[ -f ../asm_loads_check_wgrad_z.json ] || todo="$todo check:kernels_mfma_wgrad_z.hip"
[ -f ../asm_loads_check_conv_zdma.json ] || todo="$todo check:kernels_mfma_conv_z16.hip"
[ -f ../asm_loads_check_s2dma.json ] || todo="$todo check:kernels_mfma_s2.hip"
[ -f ../asm_loads_check_wgrad_zd.json ] || todo="$todo check:kernels_mfma_wgrad_zd.hip"
[ -f ../asm_loads_check_deep.json ] || todo="$todo check:kernels_mfma_deep.hip"
todo_src=$(echo $todo | tr ' ' '\n' | grep -v '^check:' | tr '\n' ' ')
if [ -n "$(echo $todo_src | tr -d ' ')" ]; then
    echo $todo_src | tr ' ' '\n' | xargs -P 6 -I{} sh -c 'f={}; hipcc '"$FLAGS"' -c "$f" -o build/${f%.*}.o'
fi
# k_mfma_conv_z and k_mfma_wgrad_z wait for inline-asm loads with hand-counted vmcnt values: check the emitted code whenever
# their file was rebuilt (tools/check_asm_loads.py: no scratch, the expected memory operations, no instruction touching a load's
# registers while it is in flight; k_deep_conv: every wave drains its sc1 partial-tile stores before the barrier in front of the
# split-K ticket); the result and the toolchain it was validated with are recorded next to the library
for pair in conv_z:kernels_mfma_conv wgrad_z:kernels_mfma_wgrad_z conv_zdma:kernels_mfma_conv_z16 s2dma:kernels_mfma_s2 wgrad_zd:kernels_mfma_wgrad_zd deep:kernels_mfma_deep; do
    which=${pair%%:*}; f=${pair##*:}
    case " $todo " in *" $f.hip "*|*" check:$f.hip "*)
        hipcc $FLAGS --cuda-device-only -S $f.hip -o build/$f.s 2>/dev/null
        python3 tools/check_asm_loads.py $which build/$f.s ../asm_loads_check_$which.json || { rm -f build/$f.o; exit 1; }
        ;;
    esac
done
# the co-registration kernels (kernels_coreg.hip), the kernels of the starts (kernels_start.hip) and those of the two lattice warps
# (kernels_warp.hip, kernels_cowarp.hip: each file's own kernels and its five instantiations of lattice_fit.h's) and of their geometry (kernels_deform.hip) and the inhomogeneity correction's (kernels_bias.hip) must not spill: read every kernel's scratch size from the compiler's resource-usage remarks whenever the file
# was rebuilt (the remarks stay in build/<file>.remarks: registers, LDS, occupancy)
for pair in kernels_coreg:10 kernels_start:6 kernels_warp:9 kernels_cowarp:9 kernels_deform:8 kernels_bias:13; do
    f=${pair%%:*}; want=${pair##*:}
    case " $todo " in *" $f.hip "*)
        hipcc $FLAGS --cuda-device-only -c -Rpass-analysis=kernel-resource-usage $f.hip -o build/$f.dev 2> build/$f.remarks
        n=$(grep -c 'ScratchSize \[bytes/lane\]: 0 ' build/$f.remarks || true)
        bad=$(grep -c 'ScratchSize \[bytes/lane\]: [1-9]' build/$f.remarks || true)
        if [ "$n" -lt "$want" ] || [ "$bad" -ne 0 ]; then
            echo "$f.hip: expected $want kernels without scratch, found $n without and $bad with (build/$f.remarks)"
            rm -f build/$f.o; exit 1
        fi
        echo "$f.hip: $n kernels, no scratch"
        ;;
    esac
done
OBJS=""
for f in $SRCS; do OBJS="$OBJS build/${f%.*}.o"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o ../libunet_hip.so $OBJS -ldl
echo "built $(cd .. && pwd)/libunet_hip.so"
