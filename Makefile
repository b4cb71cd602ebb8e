# Builds the product library (HIP, gfx950) in-tree.  `make` = product; `make oracle` = CPU checkers.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := vkfft_amd/csrc
LIBDIR := vkfft_amd/lib
# --offload-compress: the gfx950 code objects are stored zstd-compressed in the library (165 MB -> a third) and unpacked by the HIP runtime when the module loads
CXXFLAGS := -O3 -std=c++17 -fPIC -fvisibility=hidden -Iinclude -I$(CSRC) -Wno-unused-result --offload-compress
# (the parts of the mixed-radix, cyclic-convolution and convolution-row registries: the lists VKFFT_MIXED_PARTS / VKFFT_MIXCONV_PARTS / VKFFT_MIX_CONV_ROWS_PARTS / VKFFT_MIX_CONV_COLS_PARTS / VKFFT_MIX_CONV_COLS_BANK_PARTS of kernels.hip)
OBJS := $(foreach u,api planner kernels kernels_pow2 kernels_blue_r2r kernels_fused kernels_mixfused kernels_aux,build/obj/$(u).o) \
        $(foreach i,0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19,build/obj/kernels_mixed_$(i).o) $(foreach i,0 1 2 3 4 5,build/obj/kernels_mixconv_$(i).o) \
        $(foreach i,0 1 2 3 4 5 6 7,build/obj/kernels_mixconv_rows_$(i).o) $(foreach i,0 1 2 3,build/obj/kernels_mixconv_cols_$(i).o) $(foreach i,0 1 2 3,build/obj/kernels_mixconv_cols_bank_$(i).o) \
        $(foreach t,f32_row f32_col f64_row f64_col,build/obj/kernels_opfft_$(t)_0.o build/obj/kernels_opfft_$(t)_1.o) build/obj/kernels_opfft_f32_col_2.o
# the translation units that take longest to compile (12 minutes each for kernels_mixed_0 ... 5, 4-6 for the others; the rest 2 minutes or less), named first among the
# library's prerequisites so that a parallel make starts them first and no core waits for one of them at the end; the link line keeps the order of OBJS
LONG_OBJS := $(foreach i,0 1 2 3 4 5,build/obj/kernels_mixed_$(i).o) build/obj/kernels_mixconv_4.o build/obj/kernels_mixconv_0.o build/obj/kernels_mixconv_2.o \
        build/obj/kernels_opfft_f32_col_0.o build/obj/kernels_opfft_f32_col_1.o build/obj/kernels_mixconv_1.o build/obj/kernels_mixconv_3.o build/obj/kernels_mixconv_5.o \
        build/obj/kernels_opfft_f32_row_0.o build/obj/kernels_opfft_f32_row_1.o
# every rule names what it starts, so that a silent (-s) build of half an hour still shows where it stands
# header dependencies come from the compiler (-MMD): a change to one kernel family rebuilds only the translation units that include it
DEPFLAGS = -MMD -MP -MF build/obj/$*.d

all: $(LIBDIR)/libvkfft_mi355x.so build/vkfft_mi355x_cli $(if $(wildcard /opt/rocm/lib/librccl.so),build/vkfft_mi355x_multi)
multi: build/vkfft_mi355x_multi

# caller-side benchmark driver (flag-compatible in spirit with the reference's VkFFT_TestSuite): links the C-ABI only
build/vkfft_mi355x_cli: tools/vkfft_cli.cpp include/vkFFT.h $(LIBDIR)/libvkfft_mi355x.so
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Wno-unused-value -Wno-unused-result -Iinclude tools/vkfft_cli.cpp -L$(LIBDIR) -lvkfft_mi355x -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -o $@

# multi-GPU host drivers (one thread per GPU; batch sharding, slab 3D over RCCL or device-to-device copies): links the C-ABI and librccl
build/vkfft_mi355x_multi: tools/vkfft_multi.cpp include/vkFFT.h $(LIBDIR)/libvkfft_mi355x.so
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -pthread -Wno-unused-value -Wno-unused-result -Iinclude tools/vkfft_multi.cpp -L$(LIBDIR) -lvkfft_mi355x -L/opt/rocm/lib -lrccl -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib -o $@

build/obj/%.o: $(CSRC)/%.cpp
	@mkdir -p build/obj
	@echo "  HIPCC  $<"
	$(HIPCC) $(CXXFLAGS) $(DEPFLAGS) --offload-arch=$(ARCH) -c $< -o $@

build/obj/%.o: $(CSRC)/%.hip
	@mkdir -p build/obj
	@echo "  HIPCC  $<"
	$(HIPCC) $(CXXFLAGS) $(DEPFLAGS) --offload-arch=$(ARCH) -c $< -o $@

$(LIBDIR)/libvkfft_mi355x.so: $(LONG_OBJS) $(OBJS)
	@mkdir -p $(LIBDIR)
	@echo "  LINK   $@"
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(OBJS) -o $@

# development build of the fused Four-Step kernels (per-phase cycle profile, arithmetic-free variants): tools/prof_fused.py,
# selected with VKFFT_MI355X_LIB=build/libvkfft_mi355x_dev.so; never shipped
build/obj/kernels_fused_dev.o: $(CSRC)/kernels_fused.hip
	@mkdir -p build/obj
	$(HIPCC) $(CXXFLAGS) -DVKFFT_MI355X_DEV -MMD -MP -MF build/obj/kernels_fused_dev.d --offload-arch=$(ARCH) -c $< -o $@
build/libvkfft_mi355x_dev.so: $(OBJS) build/obj/kernels_fused_dev.o
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(filter-out build/obj/kernels_fused.o,$(OBJS)) build/obj/kernels_fused_dev.o -o $@
dev: build/libvkfft_mi355x_dev.so

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf build/obj $(LIBDIR)/*.so

-include $(wildcard build/obj/*.d)

.PHONY: all oracle clean dev multi
