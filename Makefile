# Builds the gfx950 C-ABI library of garage_amd (hand-written HIP kernels).
#   make            -> garage_amd/_C/libgarage_amd.so
# hipcc cross-compiles without a GPU; the .so is git-ignored but travels with
# gpurun snapshots.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CSRC  := garage_amd/csrc
OUT   := garage_amd/_C
HIPS  := gae_scan gemm skinny losses rollout policy_fused small_step fused_train narrow_step members_step lnorm member_pack linear_baseline members_diag
CPPS  := errors prof update update_members comm rollout_loop mlp_layers member_pack_host fused_train_host rollout_host losses_host linear_baseline_host linear_baseline_members_host members_diag_host
OBJS  := $(patsubst %,$(OUT)/%.o,$(HIPS) $(CPPS))
# -fno-slp-vectorize: hipcc's SLP vectorizer turns pairs of fp32 operations into packed
# VOP3P instructions and, where one operand is the high half of a register pair, sets
# OP_SEL[1] (v_pk_fma_f32 ... op_sel:[0,1,0], v_pk_mul_f32 / v_pk_add_f32 ... op_sel:[0,1]).
# On the MI355X boxes of this pool exactly that form reads a WRONG operand now and then
# while another wave of the SIMD executes v_mfma_f32_32x32x16_bf16
# (tools/mfma_valu_hazard.hip reproduces it in 100 lines).  No
# bf16 MFMA runs in the default exact-fp32 mode, but the opt-in split-operand k-loops
# and any bf16 work of another stream or process do; the library is built without
# packed fp32 altogether (same-box A/B: 108.8 ms per C3 iteration either way), and
# tests/test_isa_hazard_cpu.py scans the generated code for the form.
# -fvisibility=hidden -fvisibility-inlines-hidden: the library exports exactly what
# include/garage_amd.h declares (GA_API); tests/test_abi_cpu.py compares the two.
FLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -fno-slp-vectorize -fvisibility=hidden -fvisibility-inlines-hidden $(EXTRA)

all: $(OUT)/libgarage_amd.so $(OUT)/libgarage_amd_fused_entries.so

# (header dependencies come from the compiler: -MMD -MP writes $(OUT)/x.d beside x.o)
$(OUT)/%.o: $(CSRC)/%.hip
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -MMD -MP -c $< -o $@

$(OUT)/%.o: $(CSRC)/%.cpp
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -MMD -MP -x hip -c $< -o $@

-include $(OBJS:.o=.d)

$(OUT)/libgarage_amd.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -ldl -o $@

# For tests/test_fused_entries_strides_gpu.py only: the same objects linked a second time
# with tests/host/fused_entries_shim.cpp, which exports one wrapper around the fused
# step's forward + loss and data-gradient entry points (they are not part of the C ABI
# and stay hidden in the library itself).
$(OUT)/fused_entries_shim.o: tests/host/fused_entries_shim.cpp
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -MMD -MP -x hip -c $< -o $@

-include $(OUT)/fused_entries_shim.d

$(OUT)/libgarage_amd_fused_entries.so: $(OBJS) $(OUT)/fused_entries_shim.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) $(OUT)/fused_entries_shim.o -ldl -o $@

# developer tool: the matrix pipe's own ceiling (register-only MFMA loops)
mfma-peak: tools/mfma_peak.hip
	@mkdir -p $(OUT)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result $< -o $(OUT)/mfma_peak

# developer tools: does vector work hide behind MFMAs (fp32: no, bf16: yes), and the
# packed-fp32 / bf16-MFMA hazard reproducer
mfma-tools: tools/mfma_valu_overlap.hip tools/mfma_valu_hazard.hip tools/mfma_rounding.hip
	@mkdir -p $(OUT)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result -Wno-unused-value tools/mfma_valu_overlap.hip -o $(OUT)/mfma_valu_overlap
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result -Wno-unused-value tools/mfma_valu_hazard.hip -o $(OUT)/mfma_valu_hazard
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result -Wno-unused-value tools/mfma_rounding.hip -o $(OUT)/mfma_rounding

# the library WITH hipcc's SLP vectorizer (packed fp32, the hazardous form included):
# only for tools/hazard_repro_backward.py
slp-variant:
	@mkdir -p $(OUT)/variants/slp
	for f in $(HIPS); do $(HIPCC) $(FLAGS) -fslp-vectorize -c $(CSRC)/$$f.hip -o $(OUT)/variants/slp/$$f.o || exit 1; done
	for f in $(CPPS); do $(HIPCC) $(FLAGS) -fslp-vectorize -x hip -c $(CSRC)/$$f.cpp -o $(OUT)/variants/slp/$$f.o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OUT)/variants/slp/*.o -ldl -o $(OUT)/variants/lib_slp.so
	rm -rf $(OUT)/variants/slp

clean:
	rm -rf $(OUT)/*.o $(OUT)/*.d $(OUT)/*.so $(OUT)/asan $(OUT)/*_asan_test $(OUT)/mfma_peak $(OUT)/mfma_valu_overlap $(OUT)/mfma_valu_hazard $(OUT)/mfma_rounding $(OUT)/variants

.PHONY: all clean mfma-peak mfma-tools slp-variant

# Host-side C++ under AddressSanitizer + UBSan on the CPU (tests/host/): a harness program
# is one translation unit of tests/host/ -- recording fakes of every kernel entry point
# or launch-seam function (fused_params.h, rollout_params.h, loss_params.h, layer_plans.h,
# linear_baseline_params.h)
# and HIP call the product source makes, and the checks -- linked with that product source.
# One line per program: binary, harness source, product source (several joined by +).
ASAN_PROGRAMS := \
  host_asan_test:update_loop_harness:update \
  rollout_asan_test:rollout_loop_harness:rollout_loop \
  mlp_layers_asan_test:mlp_layers_harness:mlp_layers \
  update_members_asan_test:update_members_harness:update_members \
  member_pack_asan_test:member_pack_harness:member_pack_host \
  fused_host_asan_test:fused_host_harness:fused_train_host \
  rollout_host_asan_test:rollout_host_harness:rollout_host \
  losses_host_asan_test:losses_host_harness:losses_host \
  linear_baseline_asan_test:linear_baseline_harness:linear_baseline_host \
  linear_baseline_members_asan_test:linear_baseline_members_harness:linear_baseline_members_host \
  members_diag_asan_test:members_diag_harness:members_diag_host+mlp_layers
ASAN_CXX := g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer

# (the stem is the source's path: $(OUT)/asan/tests/host/x.o, $(OUT)/asan/$(CSRC)/y.o;
# header dependencies come from the compiler)
$(OUT)/asan/%.o: %.cpp
	@mkdir -p $(@D)
	$(ASAN_CXX) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  -MMD -MP -c $< -o $@

define asan_program
$(OUT)/$(1): $(OUT)/asan/tests/host/$(2).o $(patsubst %,$(OUT)/asan/$(CSRC)/%.o,$(subst +, ,$(3)))
	$$(ASAN_CXX) $$^ -o $$@
-include $(OUT)/asan/tests/host/$(2).d $(patsubst %,$(OUT)/asan/$(CSRC)/%.d,$(subst +, ,$(3)))
endef
$(foreach p,$(ASAN_PROGRAMS),$(eval $(call asan_program,$(word 1,$(subst :, ,$(p))),$(word 2,$(subst :, ,$(p))),$(word 3,$(subst :, ,$(p))))))

# The epoch loops (update.cpp), three suites of one program: the loops' own arithmetic;
# fused_step's slab ranges for the data-gradient launch and the optimizer launch's
# pre-summed regions; fused_step's choice between the fused forward + data-gradient
# launch and the two launches (ga_set_fused_fwd_dgrad).
asan-host: $(OUT)/host_asan_test
	$(OUT)/host_asan_test loops
asan-slab-sum: $(OUT)/host_asan_test
	$(OUT)/host_asan_test slab-sum
asan-fwd-dgrad: $(OUT)/host_asan_test
	$(OUT)/host_asan_test fwd-dgrad

# ga_rollout_env_steps' host loop (rollout_loop.cpp), two suites of one program: against a
# kernel side whose fused launch does not rescale the actions (three launches per step of
# a rescaled rollout), and against one that does, as policy_fused.hip (ONE launch, and
# three per step only under ga_set_fused_env_step(0)).
asan-env-loop: $(OUT)/rollout_asan_test
	$(OUT)/rollout_asan_test env-loop
asan-rescale-loop: $(OUT)/rollout_asan_test
	$(OUT)/rollout_asan_test rescale-loop

# The per-layer MLP dispatch (mlp_layers.cpp) with the library's kernel-choice rules
# (layer_plans.h) against fakes of the launch seam: every fake checks the extent its kernel
# would reach against the exactly-sized buffer the pointer came from and that the plan's
# grid covers the product; the plans themselves against literal tables (tile, grid,
# k_per_split, LDS bytes, variant) with both sides of every boundary.
asan-mlp: $(OUT)/mlp_layers_asan_test
	$(OUT)/mlp_layers_asan_test

# Which weight-gradient products take the paired-column GEMM (layer_plans.h:
# ga_gemm_paired_ok): a stand-alone program of the plan functions alone, one refused
# product per condition of the rule.
$(OUT)/gemm_paired_plan_check: tests/host/gemm_paired_plan_check.cpp $(CSRC)/layer_plans.h $(CSRC)/gemm_params.h
	@mkdir -p $(OUT)
	$(ASAN_CXX) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function $< -o $@
paired-plan-check: $(OUT)/gemm_paired_plan_check
	$(OUT)/gemm_paired_plan_check

# The population's epoch loop (update_members.cpp): which ids form which member's step,
# which members are active in which step, the Adam table, the launch count of a pass, the
# tables' exact sizes, nothing launched after a refusal.
asan-members: $(OUT)/update_members_asan_test
	$(OUT)/update_members_asan_test

# The joint pack's argument checks, plane table and grids (member_pack_host.cpp): every
# refusal precedes the first launch, the table's paths, units and rows, the grids' bounds.
asan-member-pack: $(OUT)/member_pack_asan_test
	$(OUT)/member_pack_asan_test

# The fused optimizer step's host side (fused_train_host.cpp) against fakes of the launch
# seam: the kernel choice against a literal table, grids, every refusal before any launch,
# the optimizer launch's virtual grid, the slab sum's offsets, the weight-plane cache.
asan-fused-host: $(OUT)/fused_host_asan_test
	$(OUT)/fused_host_asan_test

# The rollout step's host side (rollout_host.cpp) against fakes of the launch seam: the
# kernel choice, grid, member split and profile counts against a literal table, every
# refusal of every entry point before any launch for every env kind, the conversions of
# the C-ABI structs field by field, the debug hook's buffer.
asan-rollout-host: $(OUT)/rollout_host_asan_test
	$(OUT)/rollout_host_asan_test

# The host side of the stand-alone loss, statistics and optimizer kernels (losses_host.cpp)
# against fakes of the launch seam: every refusal of every entry point before any launch,
# grids, one launch or two, the parameter structs field by field, the head kernels' LDS
# bytes and the optimizer coefficients against literals.
asan-losses-host: $(OUT)/losses_host_asan_test
	$(OUT)/losses_host_asan_test

# The host side of the linear feature baseline (linear_baseline_host.cpp) against fakes of
# the launch seam: every refusal before any launch, grids that cover S on both sides of a
# slab boundary, workspace sizes, tiles per wave and LDS bytes against literals, the
# parameter structs field by field, the extents the kernels would reach.
asan-linear-baseline: $(OUT)/linear_baseline_asan_test
	$(OUT)/linear_baseline_asan_test

# The population's entries of the linear feature baseline (linear_baseline_members_host.cpp)
# against fakes of the seam: every refusal before any copy or launch, the flat grids and
# prefix tables of uneven members (one beyond the grid's cap of a lone launch included),
# each member's stretch of the workspace and the workspace bound, one table copy a call.
asan-linear-baseline-members: $(OUT)/linear_baseline_members_asan_test
	$(OUT)/linear_baseline_members_asan_test

# The population's joint diagnostics (members_diag_host.cpp) TOGETHER with the per-layer
# dispatch it asks for the members' forward plans (mlp_layers.cpp), against a fake kernel
# side of its own: every table entry against the struct the lone entry point launches for
# the same arguments, the kernel kinds and the launch count of members of different row
# counts, the members' stretches of the partials at the exact size, one table copy a call,
# every refusal before any copy or launch.
asan-members-diag: $(OUT)/members_diag_asan_test
	$(OUT)/members_diag_asan_test

# everything above; the programs with suites run all of them in one process
asan-all: $(foreach p,$(ASAN_PROGRAMS),$(OUT)/$(word 1,$(subst :, ,$(p))))
	set -e; for t in $^; do ./$$t; done

.PHONY: asan-host asan-slab-sum asan-fwd-dgrad asan-env-loop asan-rescale-loop asan-mlp \
  asan-members asan-member-pack asan-fused-host asan-rollout-host asan-losses-host \
  asan-linear-baseline asan-linear-baseline-members asan-members-diag asan-all
