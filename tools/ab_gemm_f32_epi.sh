# dev A/B of gg_gemm_nt_f32's epilogue and prologue forms on the model's shapes (run every case on ONE box: box-to-box spread is larger than most effects).
#   GG_GEMM_F32_ROWS_EPI=0                              the general epilogue instead of the row-layout one
#   GG_GEMM_F32_ROWS_EPI=0 GG_GEMM_F32_NO_PAIR_STORE=1  ... with 64-byte-run epilogue stores / loads instead of the paired whole-line ones
#   GG_GEMM_F32_PRO_RING=0                              register-staged prologue GEMMs
cd $GRAFT_REPO_ROOT
export GG_DEV_SWITCHES=1
for cfg in "" "GG_GEMM_F32_ROWS_EPI=0" "GG_GEMM_F32_ROWS_EPI=0 GG_GEMM_F32_NO_PAIR_STORE=1" "GG_GEMM_F32_PRO_RING=0"; do
  echo "== ${cfg:-default}"
  env $cfg timeout -k 10 300 python tools/bench_gemm_f32.py 2>&1 | grep -v "amdgpu.ids\|4096"
done
for cfg in "" "GG_GEMM_F32_ROWS_EPI=0" "GG_GEMM_F32_ROWS_EPI=0 GG_GEMM_F32_NO_PAIR_STORE=1"; do
  echo "== step ${cfg:-default}"
  env $cfg timeout -k 10 300 python bench.py --precision fp32 --steps 6 --warmup 2 --no-cpu-baseline --no-secondary --no-roofline 2>&1 | tail -1 | cut -c1-200
done
