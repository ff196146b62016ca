# Builds the MI355X-native graph-Laplacian filter: libglf.so (C-ABI, HIP gfx950),
# the image_processing host program and the CPU oracle used by the tests.
ROCM     ?= /opt/rocm
HIPCC    ?= $(ROCM)/bin/hipcc
ARCH     ?= gfx950
PKG      := image-processing-graph-laplacian_amd
CSRC     := $(PKG)/csrc
HOST     := $(PKG)/host
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-result -ffp-contract=fast -fno-slp-vectorize
CFLAGS   ?= -O2 -std=gnu11 -Wall -Wextra -fPIC

HIP_SRCS := $(CSRC)/ctx.hip $(CSRC)/affinity.hip $(CSRC)/eigen.hip $(CSRC)/nystroem.hip \
            $(CSRC)/filter.hip $(CSRC)/pipeline.hip $(CSRC)/comm.hip $(CSRC)/nlm.hip $(CSRC)/balance.hip \
            $(CSRC)/entrywise.hip $(CSRC)/graph.hip $(CSRC)/graph_fit.hip \
            $(CSRC)/graph_cluster.hip $(CSRC)/graph_basis.hip $(CSRC)/graph_robust.hip $(CSRC)/graph_project.hip $(CSRC)/graph_compact.hip \
            $(CSRC)/graph_quad.hip $(CSRC)/graph_edges.hip $(CSRC)/graph_classify.hip $(CSRC)/graph_softmax.hip \
            $(CSRC)/graph_blend.hip
HIP_OBJS := $(HIP_SRCS:.hip=.o)
CPP_OBJS := $(CSRC)/host_util.o
C_OBJS   := $(HOST)/png_codec.o $(HOST)/pfm_codec.o

all: $(PKG)/libglf.so $(PKG)/image_processing oracle

$(CSRC)/%.o: $(CSRC)/%.hip $(CSRC)/glf_internal.hpp $(CSRC)/phi_tile.hpp $(CSRC)/phi_compact.hpp $(CSRC)/nystroem_grid.inc $(CSRC)/nystroem_rank.inc $(CSRC)/nystroem_band.inc $(CSRC)/nystroem_band_vec.inc $(CSRC)/nystroem_band_sep.inc $(CSRC)/grid_common.inc $(CSRC)/affinity_grid.inc $(CSRC)/band_plan.hpp $(CSRC)/robust_loss.hpp $(CSRC)/filter_rule.hpp $(CSRC)/scale_rule.hpp include/glf.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/host_util.o: $(CSRC)/host_util.cpp $(CSRC)/band_plan.hpp $(CSRC)/phi_compact.hpp $(CSRC)/robust_loss.hpp include/glf.h
	$(HIPCC) -O2 -std=c++17 -fPIC -Wall -c $< -o $@

$(HOST)/%.o: $(HOST)/%.c include/glf.h $(HOST)/stages.h
	gcc $(CFLAGS) -Iinclude -c $< -o $@

$(PKG)/libglf.so: $(HIP_OBJS) $(CPP_OBJS) $(C_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ -lz -pthread -ldl

$(PKG)/image_processing: $(HOST)/image_processing.o $(HOST)/stages.o $(PKG)/libglf.so
	gcc -o $@ $(HOST)/image_processing.o $(HOST)/stages.o -L$(PKG) -lglf -Wl,-rpath,'$$ORIGIN' -lm

oracle:
	$(MAKE) -C oracle

# the PFM reader under the address and undefined-behaviour sanitizers, as a stand-alone program (CPU only)
pfm_check: tools/pfm_fuzz_main.c $(HOST)/pfm_codec.c include/glf.h
	gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -o tools/pfm_fuzz $(filter %.c,$^) -lm
	tools/pfm_fuzz

# the host-only centroid updates and k-means++ seedings (plain and weighted) under the address and undefined-behaviour sanitizers (CPU only)
cluster_check: tools/cluster_host_main.cpp $(CSRC)/host_util.cpp $(CSRC)/band_plan.hpp $(CSRC)/phi_compact.hpp $(CSRC)/robust_loss.hpp include/glf.h
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/cluster_host_check $(filter %.cpp,$^)
	tools/cluster_host_check

# the host-only change of basis (Cholesky and Ritz modes, the refusals) under the address and undefined-behaviour sanitizers (CPU only)
BASIS_CHECK_BIN ?= tools/basis_host_check
basis_check: tools/basis_host_main.cpp $(CSRC)/host_util.cpp $(CSRC)/band_plan.hpp $(CSRC)/phi_compact.hpp $(CSRC)/robust_loss.hpp include/glf.h
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o $(BASIS_CHECK_BIN) $(filter %.cpp,$^)
	$(BASIS_CHECK_BIN)

# the window plan of the fused band filter (band_rows_hull, band_cols_range, BandGeom::window) under the address and undefined-behaviour sanitizers (CPU only)
band_plan_check: tools/band_plan_host_main.cpp $(CSRC)/host_util.cpp $(CSRC)/band_plan.hpp $(CSRC)/phi_compact.hpp $(CSRC)/robust_loss.hpp include/glf.h
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/band_plan_host_check $(filter %.cpp,$^)
	tools/band_plan_host_check

# the host-only half of the robust fit (glf_robust_weight at its branch points, glf_robust_scale's median rule, every refusal) under the address and undefined-behaviour sanitizers (CPU only)
robust_check: tools/robust_host_main.cpp $(CSRC)/host_util.cpp $(CSRC)/band_plan.hpp $(CSRC)/phi_compact.hpp $(CSRC)/robust_loss.hpp include/glf.h
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/robust_host_check $(filter %.cpp,$^)
	tools/robust_host_check

# the host-only half of the compact graph handle (the exponent rule at its edges and its refusals, the folding of the column scales) under the address and undefined-behaviour sanitizers (CPU only)
compact_check: tools/compact_host_main.cpp $(CSRC)/host_util.cpp $(CSRC)/band_plan.hpp $(CSRC)/phi_compact.hpp $(CSRC)/robust_loss.hpp include/glf.h
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/compact_host_check $(filter %.cpp,$^)
	tools/compact_host_check

# the host-only half of the per-pixel quadratic forms (glf_fit_factor: the factor's identity, its determinism, every refusal) under the address and undefined-behaviour sanitizers (CPU only)
quad_check: tools/quad_host_main.cpp $(CSRC)/host_util.cpp $(CSRC)/band_plan.hpp $(CSRC)/phi_compact.hpp $(CSRC)/robust_loss.hpp include/glf.h
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/quad_host_check $(filter %.cpp,$^)
	tools/quad_host_check

# the power-of-two operand scale rule (scale_rule.hpp) against its statement in double precision, at every f32 exponent and at the edges, under the address and undefined-behaviour sanitizers (CPU only)
SCALE_RULE_CHECK_BIN ?= tools/scale_rule_host_check
scale_rule_check: tools/scale_rule_host_main.cpp $(CSRC)/scale_rule.hpp
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o $(SCALE_RULE_CHECK_BIN) $(filter %.cpp,$^)
	$(SCALE_RULE_CHECK_BIN)

clean:
	rm -f $(CSRC)/*.o $(HOST)/*.o $(PKG)/libglf.so $(PKG)/image_processing
	$(MAKE) -C oracle clean

.PHONY: all oracle clean pfm_check cluster_check basis_check band_plan_check robust_check compact_check quad_check scale_rule_check
