# Builds the gfx950 C-ABI library of garage_amd (hand-written HIP kernels).
#   make            -> garage_amd/_C/libgarage_amd.so
# hipcc cross-compiles without a GPU; the .so is git-ignored but travels with
# gpurun snapshots.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CSRC  := garage_amd/csrc
OUT   := garage_amd/_C
HIPS  := gae_scan gemm skinny losses rollout policy_fused small_step fused_train narrow_step members_step lnorm member_pack
CPPS  := errors prof update update_members comm rollout_loop mlp_layers member_pack_host
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

all: $(OUT)/libgarage_amd.so

$(OUT)/%.o: $(CSRC)/%.hip $(CSRC)/common.h $(CSRC)/internal.h $(CSRC)/prof.h $(CSRC)/small_step.h $(CSRC)/gemm_core.h $(CSRC)/gemm_params.h $(CSRC)/loss_rows.h $(CSRC)/fused_train.h $(CSRC)/rollout_dev.h $(CSRC)/narrow_body.h $(CSRC)/reduce_trees.h $(CSRC)/members_step.h $(CSRC)/member_pack.h include/garage_amd.h
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -c $< -o $@

$(OUT)/%.o: $(CSRC)/%.cpp $(CSRC)/common.h $(CSRC)/gemm_params.h $(CSRC)/internal.h $(CSRC)/prof.h $(CSRC)/small_step.h $(CSRC)/fused_train.h $(CSRC)/members_step.h $(CSRC)/member_pack.h include/garage_amd.h
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -x hip -c $< -o $@

$(OUT)/libgarage_amd.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -ldl -o $@

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
	rm -rf $(OUT)/*.o $(OUT)/*.so $(OUT)/mfma_peak $(OUT)/mfma_valu_overlap $(OUT)/mfma_valu_hazard $(OUT)/mfma_rounding $(OUT)/variants

.PHONY: all clean mfma-peak mfma-tools slp-variant

# Host-side epoch loops under AddressSanitizer + UBSan on the CPU, with every kernel
# entry point replaced by a recording fake (tests/host/).
asan-host: $(OUT)/host_asan_test
	$(OUT)/host_asan_test

$(OUT)/host_asan_test: tests/host/update_loop_harness.cpp tests/host/no_fused_fwd_dgrad.cpp $(CSRC)/update.cpp $(CSRC)/internal.h $(CSRC)/small_step.h $(CSRC)/fused_train.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/update_loop_harness.cpp tests/host/no_fused_fwd_dgrad.cpp $(CSRC)/update.cpp \
	  -o $@

.PHONY: asan-host

# ga_rollout_env_steps' host loop (rollout_loop.cpp) under AddressSanitizer +
# UBSan with recording fakes for the kernels it launches (tests/host/).
asan-env-loop: $(OUT)/env_loop_asan_test
	$(OUT)/env_loop_asan_test

$(OUT)/env_loop_asan_test: tests/host/rollout_env_loop_harness.cpp tests/host/no_rescale_in_launch.cpp $(CSRC)/rollout_loop.cpp $(CSRC)/internal.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/rollout_env_loop_harness.cpp tests/host/no_rescale_in_launch.cpp \
	  $(CSRC)/rollout_loop.cpp -o $@

.PHONY: asan-env-loop

# The same loop against a kernel side that rescales the actions inside the fused launch,
# as policy_fused.hip does: a rescaled rollout is ONE launch, and three per step only
# under ga_set_fused_env_step(0) (tests/host/).  The harness above links a kernel side
# that does not (no_rescale_in_launch.cpp) and pins the three launches.
asan-rescale-loop: $(OUT)/rescale_loop_asan_test
	$(OUT)/rescale_loop_asan_test

$(OUT)/rescale_loop_asan_test: tests/host/rollout_rescale_loop_harness.cpp $(CSRC)/rollout_loop.cpp $(CSRC)/internal.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/rollout_rescale_loop_harness.cpp $(CSRC)/rollout_loop.cpp \
	  -o $@

.PHONY: asan-rescale-loop

# The per-layer MLP dispatch (mlp_layers.cpp) under AddressSanitizer + UBSan with
# recording fakes for the launches it makes; every fake checks the extent its kernel
# would reach against the exactly-sized buffer the pointer came from (tests/host/).
asan-mlp: $(OUT)/mlp_layers_asan_test
	$(OUT)/mlp_layers_asan_test

$(OUT)/mlp_layers_asan_test: tests/host/mlp_layers_harness.cpp $(CSRC)/mlp_layers.cpp $(CSRC)/common.h $(CSRC)/gemm_params.h $(CSRC)/internal.h $(CSRC)/fused_train.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/mlp_layers_harness.cpp $(CSRC)/mlp_layers.cpp \
	  -o $@

.PHONY: asan-mlp

# fused_step's slab ranges for the data-gradient launch and the optimizer launch's
# pre-summed regions (update.cpp) under AddressSanitizer + UBSan, with fakes that walk
# the ranges inside an exactly-sized slab workspace (tests/host/).
asan-slab-sum: $(OUT)/slab_sum_asan_test
	$(OUT)/slab_sum_asan_test

$(OUT)/slab_sum_asan_test: tests/host/slab_sum_harness.cpp tests/host/no_fused_fwd_dgrad.cpp $(CSRC)/update.cpp $(CSRC)/internal.h $(CSRC)/small_step.h $(CSRC)/fused_train.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/slab_sum_harness.cpp tests/host/no_fused_fwd_dgrad.cpp $(CSRC)/update.cpp \
	  -o $@

.PHONY: asan-slab-sum

# fused_step's choice between the fused forward + data-gradient launch and the two
# launches (update.cpp, ga_set_fused_fwd_dgrad) under AddressSanitizer + UBSan: the order
# of the launches on a stream, no slab ranges and no pre-summed regions with the fused
# launch, the old sequence wherever it does not apply (tests/host/).  The two harnesses
# above link a kernel side WITHOUT the fused instantiation (no_fused_fwd_dgrad.cpp) and
# pin the two-launch sequence.
asan-fwd-dgrad: $(OUT)/fused_fwd_dgrad_asan_test
	$(OUT)/fused_fwd_dgrad_asan_test

$(OUT)/fused_fwd_dgrad_asan_test: tests/host/fused_fwd_dgrad_harness.cpp $(CSRC)/update.cpp $(CSRC)/internal.h $(CSRC)/small_step.h $(CSRC)/fused_train.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/fused_fwd_dgrad_harness.cpp $(CSRC)/update.cpp \
	  -o $@

.PHONY: asan-fwd-dgrad

# The population's epoch loop (update_members.cpp) under AddressSanitizer + UBSan with
# recording fakes for its two launches and the HIP calls it makes: which ids form which
# member's step, which members are active in which step, the Adam table, the launch
# count of a pass, the tables' exact sizes, nothing launched after a refusal
# (tests/host/).
asan-members: $(OUT)/update_members_asan_test
	$(OUT)/update_members_asan_test

$(OUT)/update_members_asan_test: tests/host/update_members_harness.cpp $(CSRC)/update_members.cpp $(CSRC)/common.h $(CSRC)/internal.h $(CSRC)/members_step.h $(CSRC)/fused_train.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/update_members_harness.cpp $(CSRC)/update_members.cpp \
	  -o $@

.PHONY: asan-members

# The joint pack's argument checks, plane table and grids (member_pack_host.cpp) under
# AddressSanitizer + UBSan with recording fakes for its three launches: every refusal
# precedes the first launch, the table's paths, units and rows, the grids' bounds
# (tests/host/).
asan-member-pack: $(OUT)/member_pack_asan_test
	$(OUT)/member_pack_asan_test

$(OUT)/member_pack_asan_test: tests/host/member_pack_harness.cpp $(CSRC)/member_pack_host.cpp $(CSRC)/common.h $(CSRC)/internal.h $(CSRC)/member_pack.h include/garage_amd.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
	  -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function \
	  tests/host/member_pack_harness.cpp $(CSRC)/member_pack_host.cpp \
	  -o $@

.PHONY: asan-member-pack
