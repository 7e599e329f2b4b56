// Build-only probe: the register / scratch / occupancy table of the one-launch MLP step family.  Nothing runs.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Wno-pass-failed -Wno-inline-asm -I i-dqn_amd/csrc -I include \
//         --cuda-device-only -Rpass-analysis=kernel-resource-usage -c tools/probes/fc_step_resources.hip -o /dev/null
// The template kernels are instantiated here (the stamped single step once); k_fc_group_step / k_fc_group_steps are plain kernels of the header.  A
// change to the family keeps ScratchSize at 0, the occupancy, and VGPRs no higher than before ("Resources").
#include "fc_group_kernels.h"

template __global__ void k_fc_step_par<false, FcBatchSrc>(FcArgs, FcParPlan, AdamConsts, float*, float*, float*, int, FcBatchSrc);
template __global__ void k_fc_step_par<false, FcRingSrc<RpsSlotsPar>>(FcArgs, FcParPlan, AdamConsts, float*, float*, float*, int, FcRingSrc<RpsSlotsPar>);
template __global__ void k_fc_step_par<false, FcRingSrc<RpsSlotsDev>>(FcArgs, FcParPlan, AdamConsts, float*, float*, float*, int, FcRingSrc<RpsSlotsDev>);
template __global__ void k_fc_step_par<true, FcRingSrc<RpsSlotsDev>>(FcArgs, FcParPlan, AdamConsts, float*, float*, float*, int, FcRingSrc<RpsSlotsDev>);
template __global__ void k_fc_steps_par<FcRingSrc<RpsSlotsDev>>(FcArgs, FcParPlan, AdamConsts, float*, float*, float*, int, FcRingSrc<RpsSlotsDev>);
