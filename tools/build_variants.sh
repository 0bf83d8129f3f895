#!/bin/bash
# Profiling-only builds of libdlsa_hip.so with DLSA_ABLATE=1/2/3 (see
# dlsa_amd/csrc/irls_coop_impl.hpp; nt / sc1: cache policy of the X stream).  Output: var/*.so (git-ignored, travels to the GPU box).
set -e
mkdir -p var
cd "$(dirname "$0")/.."
for v in "$@"; do
  case $v in
    ablate1) D=DLSA_ABLATE=1 ;;
    ablate2) D=DLSA_ABLATE=2 ;;
    ablate3) D=DLSA_ABLATE=3 ;;
    ablate4) D=DLSA_ABLATE=4 ;;
    cat1) D=DLSA_CAT_ABLATE=1 ;;
    cat2) D=DLSA_CAT_ABLATE=2 ;;
    cat4) D=DLSA_CAT_ABLATE=4 ;;
    cat7) D=DLSA_CAT_ABLATE=7 ;;
    cat15) D=DLSA_CAT_ABLATE=15 ;;
    cat16) D=DLSA_CAT_ABLATE=16 ;;
    cat8) D=DLSA_CAT_ABLATE=8 ;;
    cat32) D=DLSA_CAT_ABLATE=32 ;;
    solveprof) D=DLSA_SOLVE_PROFILE=1 ;;
    cat31) D=DLSA_CAT_ABLATE=31 ;;
    fab1) D=DLSA_FUSED_ABLATE=1 ;;
    ozprof) D=DLSA_OZ_PROF=1 ;;
    ozcheck) D=DLSA_OZ_CHECK=1 ;;
    knobs) D=DLSA_ENV_KNOBS=1 ;;
    cmabl) D=DLSA_CM_ABLATE=1 ;;
    wnprof) D=DLSA_WN_PROF=1 ;;
    nt) D=DLSA_X_DMA_AUX=2 ;;
    dma0) D=DLSA_X_DMA_AUX=0 ;;
    sc1) D=DLSA_X_DMA_AUX=1 ;;
    coopdma0) D=DLSA_COOP_NT7_DMA_AUX=0 ;;  # the NT = 7 bf16 cooperative pass at the default policy
    coopnt) D=DLSA_X_DMA_AUX=2 ;;  # every NT of the logistic / OLS cooperative pass non-temporal
    *) echo "unknown variant $v"; exit 1 ;;
  esac
  ONLY=None
  # the planning header (fit_plan.hpp: env_knob) is compiled into all of these
  HOST='"fit_fused.hip", "fit_wide.hip", "fit_cat.hip", "capi.hip"'
  case $v in
    oz*) ONLY='["irls_oz.hip", "irls_oz_g2.hip"]' ;;
    solve*) ONLY='["newton_solve.hip"]' ;;
    cat*) ONLY='["cat_pass.hip"]' ;;
    wn*) ONLY='["wide_newton.hip"]' ;;
    fab1) ONLY='["wide_fused.hip"]' ;;
    knobs) ONLY="[$HOST]" ;;
    cmabl|coopdma0|coopnt) ONLY='["irls_coop_g1.hip", "irls_coop_g2.hip", "irls_coop_g3.hip", "irls_coop_g4.hip", "irls_coop_g5.hip", "irls_coop_g6.hip"]' ;;
  esac
  python -c "from dlsa_amd.build import build; print(build(force=True, out='var/libdlsa_hip_$v.so', defines='$D'.replace('-D', '').split(), only=$ONLY))"
done
