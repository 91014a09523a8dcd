# Build of the MI355X SASA engine (gfx950 only).
#   make            -> freesasa_amd/lib/libfreesasa_amd.so (stand-alone drop-in library)
#                      freesasa_amd/lib/libfreesasa_amd_seam.a (seam objects for a drop-in
#                      build of the reference)
#   make emu        -> tests/emu/libsasa_emu.so, libselect_emu.so, libgroups_emu.so, libtraj_emu.so, libtraj_groups_emu.so, libtraj_pairs_emu.so, libtraj_pair_res_emu.so, libdcd_emu.so, libnc_emu.so, libxtc_emu.so, libtrr_emu.so, libpbc_emu.so, libpbc_tri_emu.so, libgroups_pbc_emu.so, libtraj_pairs_pbc_emu.so, libstats_emu.so, libvolume_emu.so, libdots_emu.so, libiface_emu.so, libiface_res_emu.so, libcontacts_emu.so, librescontacts_emu.so, libifsweep_emu.so, libocc_emu.so  (TESTS ONLY: the kernel phase
#                      functions driven on the CPU; never linked into the product) and tests/emu/dcd_check, tests/emu/cell_check, tests/emu/nc_check, tests/emu/xtc_check, tests/emu/xtc_emu_check, tests/emu/trr_check, tests/emu/stats_check, tests/emu/dots_check, tests/emu/iface_check, tests/emu/iface_res_check, tests/emu/contacts_check, tests/emu/rescontacts_check, tests/emu/ifsweep_check, tests/emu/occ_check, tests/emu/groups_pbc_check, tests/emu/pair_res_check (the DCD, NetCDF, XTC and TRR header parsers, the cell arithmetic, the emulated XTC decode, the merge of the run statistics and the emulated scan and expansion of the surface dots and the emulated phases of the interfaces between chain groups and of their per-residue, atom-atom contact and residue-residue contact tables and of the file sweep's interface kernels and of the contact occupancy map and the segments and rows of the per-residue interface tables per frame under sanitizers) and tests/emu/ingest_check (the host loader's PDB / mmCIF parsers under sanitizers)
#   make oracle     -> oracle/ (TESTS ONLY) ; make tools -> tools/libsasa_synth.so
HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
CXX     ?= g++
ARCH    ?= gfx950
CSRC     = freesasa_amd/csrc
LIBDIR   = freesasa_amd/lib
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function
CFLAGS   = -O2 -std=gnu99 -fPIC -ffp-contract=off -Wall

all: $(LIBDIR)/libfreesasa_amd.so $(LIBDIR)/libfreesasa_amd_seam.a

# Device code lives in ONE translation unit (gpu_kernels.hip); the compiler's per-kernel resource report (registers,
# scratch, LDS) is kept next to its object: tests/test_capi.py checks that the hot kernels do not spill.  The other
# .hip files are host code over the HIP runtime (engine_internal.h says who holds what).
ENGINE_HDRS = $(CSRC)/classifier.h $(CSRC)/engine_internal.h $(CSRC)/sasa_kernels.h $(CSRC)/group_kernels.h $(CSRC)/select_kernels.h $(CSRC)/traj_kernels.h $(CSRC)/xtc_kernels.h $(CSRC)/pbc_kernels.h $(CSRC)/pbc_tri_kernels.h $(CSRC)/vol_kernels.h $(CSRC)/dots_kernels.h $(CSRC)/iface_kernels.h $(CSRC)/contact_kernels.h $(CSRC)/rescontact_kernels.h $(CSRC)/ifsweep_kernels.h $(CSRC)/occupancy_kernels.h $(CSRC)/select_program.h $(CSRC)/sr_caps.h $(CSRC)/lr2_kernels.h $(CSRC)/kat_kernels.h $(CSRC)/gpu_parse.h $(CSRC)/protor_table.h include/freesasa_gpu.h include/freesasa_ingest.h
$(LIBDIR)/gpu_kernels.o: $(CSRC)/gpu_kernels.hip $(ENGINE_HDRS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(LIBDIR)/kernel_resources.txt; rc=$$?; \
	grep -v "remark:" $(LIBDIR)/kernel_resources.txt >&2; exit $$rc
$(LIBDIR)/gpu_%.o: $(CSRC)/gpu_%.hip $(ENGINE_HDRS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
GPU_OBJS = $(LIBDIR)/gpu_kernels.o $(LIBDIR)/gpu_engine.o $(LIBDIR)/gpu_ops.o $(LIBDIR)/gpu_hostbatch.o $(LIBDIR)/gpu_drivers.o $(LIBDIR)/gpu_frames.o $(LIBDIR)/gpu_sweep.o $(LIBDIR)/gpu_parse.o $(LIBDIR)/gpu_groups.o $(LIBDIR)/gpu_periodic.o $(LIBDIR)/gpu_volume.o $(LIBDIR)/gpu_dots.o $(LIBDIR)/gpu_interfaces.o $(LIBDIR)/gpu_occupancy.o

$(LIBDIR)/seam.o: $(CSRC)/seam.c include/freesasa_amd.h include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/testpoints.o: $(CSRC)/testpoints.c include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/dcd.o: $(CSRC)/dcd.c include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/netcdf.o: $(CSRC)/netcdf.c include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/xtc.o: $(CSRC)/xtc.c include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/trr.o: $(CSRC)/trr.c include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/cell.o: $(CSRC)/cell.c include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/trajstats.o: $(CSRC)/trajstats.c include/freesasa_gpu.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/api.o: $(CSRC)/api.c include/freesasa_amd.h $(CSRC)/hostfault.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

# host-side fault injection (tests): the countdown every allocation / thread creation of the host code asks, and - in
# the shared library ONLY, never in the seam archive that is linked into the reference's build - the library-local
# operator new that puts the engine's C++ allocations behind it (hostfault.h)
$(LIBDIR)/hostfault.o: $(CSRC)/hostfault.c $(CSRC)/hostfault.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@
$(LIBDIR)/hostfault_new.o: $(CSRC)/hostfault_new.cpp $(CSRC)/hostfault.h
	@mkdir -p $(LIBDIR)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -c $< -o $@

$(LIBDIR)/ingest.o: $(CSRC)/ingest.c $(CSRC)/protor_table.h $(CSRC)/classifier.h include/freesasa_ingest.h $(CSRC)/hostfault.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -Iinclude -pthread -c $< -o $@

$(LIBDIR)/classifier.o: $(CSRC)/classifier.c $(CSRC)/classifier.h include/freesasa_ingest.h $(CSRC)/hostfault.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -Iinclude -c $< -o $@

$(LIBDIR)/select.o: $(CSRC)/select.c $(CSRC)/select_program.h include/freesasa_ingest.h $(CSRC)/hostfault.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -Iinclude -c $< -o $@

$(LIBDIR)/ingest_cache.o: $(CSRC)/ingest_cache.c include/freesasa_ingest.h $(CSRC)/hostfault.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -Iinclude -pthread -c $< -o $@

$(LIBDIR)/libfreesasa_amd.so: $(GPU_OBJS) $(LIBDIR)/seam.o $(LIBDIR)/testpoints.o $(LIBDIR)/dcd.o $(LIBDIR)/netcdf.o $(LIBDIR)/xtc.o $(LIBDIR)/trr.o $(LIBDIR)/cell.o $(LIBDIR)/trajstats.o $(LIBDIR)/api.o $(LIBDIR)/ingest.o $(LIBDIR)/classifier.o $(LIBDIR)/select.o $(LIBDIR)/ingest_cache.o $(LIBDIR)/hostfault.o $(LIBDIR)/hostfault_new.o $(CSRC)/exports.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--version-script=$(CSRC)/exports.map -o $@ $(filter %.o,$^)

$(LIBDIR)/libfreesasa_amd_seam.a: $(GPU_OBJS) $(LIBDIR)/seam.o $(LIBDIR)/testpoints.o $(LIBDIR)/dcd.o $(LIBDIR)/netcdf.o $(LIBDIR)/xtc.o $(LIBDIR)/trr.o $(LIBDIR)/cell.o $(LIBDIR)/trajstats.o $(LIBDIR)/ingest.o $(LIBDIR)/classifier.o $(LIBDIR)/select.o $(LIBDIR)/ingest_cache.o $(LIBDIR)/hostfault.o
	rm -f $@; ar rcs $@ $^

emu: tests/emu/libsasa_emu.so tests/emu/libingest_scalar.so tests/emu/libselect_emu.so tests/emu/libgroups_emu.so tests/emu/libtraj_emu.so tests/emu/libtraj_groups_emu.so tests/emu/libtraj_pairs_emu.so tests/emu/libtraj_pair_res_emu.so tests/emu/pair_res_check tests/emu/libdcd_emu.so tests/emu/libpbc_emu.so tests/emu/libpbc_tri_emu.so tests/emu/libgroups_pbc_emu.so tests/emu/libtraj_pairs_pbc_emu.so tests/emu/libnc_emu.so tests/emu/libxtc_emu.so tests/emu/libtrr_emu.so tests/emu/libstats_emu.so tests/emu/libvolume_emu.so tests/emu/libdots_emu.so tests/emu/dcd_check tests/emu/cell_check tests/emu/nc_check tests/emu/xtc_check tests/emu/xtc_emu_check tests/emu/trr_check tests/emu/stats_check tests/emu/dots_check tests/emu/libiface_emu.so tests/emu/iface_check tests/emu/libiface_res_emu.so tests/emu/iface_res_check tests/emu/libcontacts_emu.so tests/emu/contacts_check tests/emu/librescontacts_emu.so tests/emu/rescontacts_check tests/emu/libifsweep_emu.so tests/emu/ifsweep_check tests/emu/libocc_emu.so tests/emu/occ_check tests/emu/groups_pbc_check tests/emu/ingest_check
# the loader with its byte-at-a-time mmCIF tokenizer only: the differential twin of the SSE2 row scanner
tests/emu/libingest_scalar.so: $(CSRC)/ingest.c $(CSRC)/classifier.c $(CSRC)/classifier.h $(CSRC)/hostfault.c $(CSRC)/hostfault.h $(CSRC)/protor_table.h include/freesasa_ingest.h
	$(CC) $(CFLAGS) -DFREESASA_INGEST_NO_SIMD -Iinclude -pthread -shared -o $@ $(CSRC)/ingest.c $(CSRC)/classifier.c $(CSRC)/hostfault.c -lm
# ... and the loader's parsers under AddressSanitizer + UBSan in a stand-alone program: every text in a block of exactly its size, one line per file of argv
tests/emu/ingest_check: tests/emu/ingest_check.c $(CSRC)/ingest.c $(CSRC)/classifier.c $(CSRC)/classifier.h $(CSRC)/hostfault.c $(CSRC)/hostfault.h $(CSRC)/protor_table.h include/freesasa_ingest.h
	$(CC) -O1 -g -std=gnu99 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Iinclude -pthread -o $@ tests/emu/ingest_check.c $(CSRC)/ingest.c $(CSRC)/classifier.c $(CSRC)/hostfault.c -lm
tests/emu/libsasa_emu.so: tests/emu/emu.cpp $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h $(CSRC)/lr2_kernels.h $(CSRC)/kat_kernels.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu.cpp -lm

# the selection kernels' phase functions (select_kernels.h) driven over a loaded batch
tests/emu/libselect_emu.so: tests/emu/emu_select.cpp $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/sasa_kernels.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_select.cpp -lm

# the trajectory topology's phase functions (traj_kernels.h): the gather and the per-frame sums over one structure of a loaded batch
tests/emu/libtraj_emu.so: tests/emu/emu_traj.cpp $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/sasa_kernels.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_traj.cpp -lm

# DCD input (traj_kernels.h, traj_gather_dcd): the bytes of a file's frames -> compact fp64 frames
tests/emu/libdcd_emu.so: tests/emu/emu_dcd.cpp $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/sasa_kernels.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_dcd.cpp -lm
# AMBER NetCDF input (traj_kernels.h, traj_gather_nc): the bytes of a file's records -> compact fp64 frames
tests/emu/libnc_emu.so: tests/emu/emu_nc.cpp $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/sasa_kernels.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_nc.cpp -lm
# XTC input (xtc_kernels.h, xtc_scan and xtc_unpack): the bytes of a file's frames -> group records and raw fp32 frames; the
# descriptors through xtc.c, as the driver makes them
tests/emu/libxtc_emu.so: tests/emu/emu_xtc.cpp $(CSRC)/xtc.c $(CSRC)/xtc_kernels.h $(CSRC)/sasa_kernels.h include/freesasa_gpu.h
	$(CC) $(CFLAGS) -c $(CSRC)/xtc.c -o tests/emu/xtc_emu.o
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_xtc.cpp tests/emu/xtc_emu.o -lm
# TRR input (traj_kernels.h, traj_gather_trr): the bytes of a file's records -> compact fp64 frames; x_off through trr.c, as the
# driver makes it
tests/emu/libtrr_emu.so: tests/emu/emu_trr.cpp $(CSRC)/trr.c $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/sasa_kernels.h include/freesasa_gpu.h include/freesasa_ingest.h
	$(CC) $(CFLAGS) -c $(CSRC)/trr.c -o tests/emu/trr_emu.o
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_trr.cpp tests/emu/trr_emu.o -lm
# periodic images (pbc_kernels.h): count, emit and collect, the 256 threads of a workgroup as fibers in lock step
tests/emu/libpbc_emu.so: tests/emu/emu_pbc.cpp $(CSRC)/pbc_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_pbc.cpp -lm
# ... in a triclinic cell (pbc_tri_kernels.h): count and emit
tests/emu/libpbc_tri_emu.so: tests/emu/emu_pbc_tri.cpp tests/emu/emu_pbc.cpp $(CSRC)/pbc_tri_kernels.h $(CSRC)/pbc_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_pbc_tri.cpp -lm
# ... chain groups among periodic images (pbc_kernels.h, GpbcArgs): the combined structures' cells and the fused collect-and-finish
tests/emu/libgroups_pbc_emu.so: tests/emu/emu_groups_pbc.cpp tests/emu/emu_pbc_tri.cpp tests/emu/emu_pbc.cpp $(CSRC)/pbc_tri_kernels.h $(CSRC)/pbc_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_groups_pbc.cpp -lm
# ... with the pair part of a trajectory shard's combined batch (interfaces among periodic images: GpbcArgs' k_fixed)
tests/emu/libtraj_pairs_pbc_emu.so: tests/emu/emu_traj_pairs_pbc.cpp tests/emu/emu_groups_pbc.cpp tests/emu/emu_pbc_tri.cpp tests/emu/emu_pbc.cpp $(CSRC)/pbc_tri_kernels.h $(CSRC)/pbc_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_traj_pairs_pbc.cpp -lm
# ... and the same phases (emu_groups_pbc.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per stage
tests/emu/groups_pbc_check: tests/emu/emu_groups_pbc.cpp tests/emu/emu_pbc_tri.cpp tests/emu/emu_pbc.cpp $(CSRC)/pbc_tri_kernels.h $(CSRC)/pbc_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DGPBC_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_groups_pbc.cpp -lm
# run statistics (traj_kernels.h, traj_stats): a shard's partial of the blocks of its outputs
# molecular volume (vol_kernels.h): the structures' origins, the atoms' terms, the totals over them; and emu.cpp once more, its store phase the volume's
tests/emu/libvolume_emu.so: tests/emu/emu_volume.cpp tests/emu/emu.cpp $(CSRC)/vol_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h $(CSRC)/lr2_kernels.h $(CSRC)/kat_kernels.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_volume.cpp -lm
# surface dots (dots_kernels.h): the scan of the masks' popcounts and the expansion; and emu.cpp once more, its store phase the one that keeps the masks
tests/emu/libdots_emu.so: tests/emu/emu_dots.cpp tests/emu/emu.cpp $(CSRC)/dots_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h $(CSRC)/lr2_kernels.h $(CSRC)/kat_kernels.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_dots.cpp -lm
# ... and scan and expansion (emu_dots.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/dots_check: tests/emu/emu_dots.cpp $(CSRC)/dots_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DDOTS_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_dots.cpp -lm
# interfaces between chain groups (iface_kernels.h): boxes, candidates, exact contact, gather and finish, the threads of a workgroup as fibers in lock step
tests/emu/libiface_emu.so: tests/emu/emu_iface.cpp $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_iface.cpp -lm
# ... and the same phases (emu_iface.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/iface_check: tests/emu/emu_iface.cpp $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DIFACE_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_iface.cpp -lm
# ... their per-residue tables (iface_kernels.h, IfaceResArgs): heads, the block scan, segments and rows
tests/emu/libiface_res_emu.so: tests/emu/emu_iface_res.cpp $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_iface_res.cpp -lm
# ... and the same phases (emu_iface_res.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/iface_res_check: tests/emu/emu_iface_res.cpp $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DIFACE_RES_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_iface_res.cpp -lm
# ... their atom-atom contact tables (contact_kernels.h): the buried masks, the dots' scan and expansion, the partners (the threads of a workgroup as fibers in lock step) and the rows
tests/emu/libcontacts_emu.so: tests/emu/emu_contacts.cpp $(CSRC)/contact_kernels.h $(CSRC)/dots_kernels.h $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_contacts.cpp -lm
# ... and the same phases (emu_contacts.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/contacts_check: tests/emu/emu_contacts.cpp $(CSRC)/contact_kernels.h $(CSRC)/dots_kernels.h $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DCONTACTS_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_contacts.cpp -lm
# ... their residue-residue contact tables (rescontact_kernels.h): the segments by the per-residue tables' phases, the fold (the lanes of a wave as fibers in lock step) and the reverse rows
tests/emu/librescontacts_emu.so: tests/emu/emu_rescontacts.cpp $(CSRC)/rescontact_kernels.h $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_rescontacts.cpp -lm
# ... and the same phases (emu_rescontacts.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/rescontacts_check: tests/emu/emu_rescontacts.cpp $(CSRC)/rescontact_kernels.h $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DRESCONTACTS_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_rescontacts.cpp -lm
# ... in the file sweep (ifsweep_kernels.h): the classes of the pair structures' atoms with the class sums of the sides behind them, the rows' place and labels
tests/emu/libifsweep_emu.so: tests/emu/emu_ifsweep.cpp $(CSRC)/ifsweep_kernels.h $(CSRC)/sasa_kernels.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_ifsweep.cpp -lm
# ... and the same phases (emu_ifsweep.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/ifsweep_check: tests/emu/emu_ifsweep.cpp $(CSRC)/ifsweep_kernels.h $(CSRC)/sasa_kernels.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DIFSWEEP_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_ifsweep.cpp -lm
# the residue contact occupancy map (occupancy_kernels.h): the keys of a chunk, the first occurrences with the block scan, the merge by ranks, the accumulation and the reverse rows
tests/emu/libocc_emu.so: tests/emu/emu_occupancy.cpp $(CSRC)/occupancy_kernels.h $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -shared -o $@ tests/emu/emu_occupancy.cpp -lm
# ... and the same phases (emu_occupancy.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/occ_check: tests/emu/emu_occupancy.cpp $(CSRC)/occupancy_kernels.h $(CSRC)/iface_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DOCC_CHECK_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_occupancy.cpp -lm

tests/emu/libstats_emu.so: tests/emu/emu_stats.cpp $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/sasa_kernels.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_stats.cpp -lm
# ... and the merge of the partials (trajstats.c) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/stats_check: tests/emu/stats_check.c $(CSRC)/trajstats.c include/freesasa_gpu.h
	$(CC) -O1 -g -std=gnu99 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/stats_check.c $(CSRC)/trajstats.c -lm
# the DCD header parser (dcd.c) under AddressSanitizer + UBSan in a stand-alone program: one line per file of argv
tests/emu/dcd_check: tests/emu/dcd_check.c $(CSRC)/dcd.c include/freesasa_gpu.h
	$(CC) -O1 -g -std=gnu99 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/dcd_check.c $(CSRC)/dcd.c
# the host arithmetic of triclinic cells (cell.c) likewise: one line per cell record of argv
tests/emu/cell_check: tests/emu/cell_check.c $(CSRC)/cell.c include/freesasa_gpu.h
	$(CC) -O1 -g -std=gnu99 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/cell_check.c $(CSRC)/cell.c -lm
# the AMBER NetCDF header parser (netcdf.c) and the cell decoding behind it (cell.c) likewise: one line per file of argv
tests/emu/nc_check: tests/emu/nc_check.c $(CSRC)/netcdf.c $(CSRC)/cell.c include/freesasa_gpu.h
	$(CC) -O1 -g -std=gnu99 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/nc_check.c $(CSRC)/netcdf.c $(CSRC)/cell.c -lm
# the XTC header walker (xtc.c) likewise: one line per file of argv
tests/emu/xtc_check: tests/emu/xtc_check.c $(CSRC)/xtc.c include/freesasa_gpu.h
	$(CC) -O1 -g -std=gnu99 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/xtc_check.c $(CSRC)/xtc.c -lm
# the TRR header walker (trr.c) likewise: one line per file of argv
tests/emu/trr_check: tests/emu/trr_check.c $(CSRC)/trr.c include/freesasa_gpu.h
	$(CC) -O1 -g -std=gnu99 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/trr_check.c $(CSRC)/trr.c -lm
# ... and the emulated XTC decode kernels behind it (emu_xtc.cpp with its main): one line per frame of the files of argv
tests/emu/xtc_emu_check: tests/emu/emu_xtc.cpp $(CSRC)/xtc.c $(CSRC)/xtc_kernels.h $(CSRC)/sasa_kernels.h include/freesasa_gpu.h
	$(CC) -O1 -g -std=gnu99 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -c $(CSRC)/xtc.c -o tests/emu/xtc_san.o
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DXTC_EMU_MAIN -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_xtc.cpp tests/emu/xtc_san.o -lm

# chain groups per frame (traj_kernels.h, traj_group_*) and, as their yardstick, the chain-group entry's phase functions
# (group_kernels.h) on one frame as a batch of one structure
tests/emu/libtraj_groups_emu.so: tests/emu/emu_traj_groups.cpp $(CSRC)/traj_kernels.h $(CSRC)/group_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_traj_groups.cpp -lm
# interfaces between chain groups per frame (traj_kernels.h, traj_pair_*) behind the groups' phases, in the driver's launch order
tests/emu/libtraj_pairs_emu.so: tests/emu/emu_traj_pairs.cpp $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_traj_pairs.cpp -lm
# ... and their per-residue tables (traj_kernels.h, traj_pair_res_cut and traj_pair_res): the segments on the host, the rows in the kernel's grid
tests/emu/libtraj_pair_res_emu.so: tests/emu/emu_traj_pair_res.cpp $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_traj_pair_res.cpp -lm
# ... and the same (emu_traj_pair_res.cpp with its main) under AddressSanitizer + UBSan in a stand-alone program: one line per case
tests/emu/pair_res_check: tests/emu/emu_traj_pair_res.cpp $(CSRC)/traj_kernels.h $(CSRC)/select_kernels.h $(CSRC)/select_program.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h include/freesasa_ingest.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -ffp-contract=off -DSASA_EMU -DPAIR_RES_CHECK_MAIN -Iinclude -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o $@ tests/emu/emu_traj_pair_res.cpp -lm

# the group-ids kernel's phase function (group_kernels.h, gid_struct) driven over a loaded batch, one wave per structure
tests/emu/libgroups_emu.so: tests/emu/emu_groups.cpp $(CSRC)/group_kernels.h $(CSRC)/lr2_kernels.h $(CSRC)/sasa_kernels.h $(CSRC)/sr_caps.h include/freesasa_ingest.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -DSASA_EMU -Iinclude -shared -o $@ tests/emu/emu_groups.cpp -lm

# Sanitizer build of the HOST sources (the reference's CI runs its C under sanitizers): the parsers,
# the selection language, the C API shims and the test-point generator with AddressSanitizer + UBSan, linked with
# the ordinary (uninstrumented) engine object; its objects stay in the tree (tests/emu/asan_*.o), so that builds by
# different users of one machine do not share them.  `make asan-test` runs the CPU suites that exercise them.
ASAN_SO = tests/emu/libfreesasa_amd_asan.so
SANFLAGS = -O1 -g -std=gnu99 -fPIC -ffp-contract=off -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
asan: $(ASAN_SO)
$(ASAN_SO): $(CSRC)/api.c $(CSRC)/seam.c $(CSRC)/testpoints.c $(CSRC)/dcd.c $(CSRC)/netcdf.c $(CSRC)/xtc.c $(CSRC)/trr.c $(CSRC)/cell.c $(CSRC)/trajstats.c $(CSRC)/ingest.c $(CSRC)/classifier.c $(CSRC)/classifier.h $(CSRC)/select.c $(CSRC)/ingest_cache.c $(CSRC)/hostfault.c $(CSRC)/hostfault.h $(CSRC)/protor_table.h $(GPU_OBJS) include/freesasa_amd.h include/freesasa_gpu.h include/freesasa_ingest.h
	for f in api seam testpoints dcd netcdf xtc trr cell trajstats ingest classifier select ingest_cache hostfault; do $(CC) $(SANFLAGS) -Iinclude -pthread -c $(CSRC)/$$f.c -o tests/emu/asan_$$f.o || exit 1; done
	$(CXX) -shared -fPIC -o $@ $(foreach f,api seam testpoints dcd netcdf xtc trr cell trajstats ingest classifier select ingest_cache hostfault,tests/emu/asan_$(f).o) $(GPU_OBJS) \
	    -fsanitize=address,undefined -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64 -lpthread -lm
asan-test: $(ASAN_SO) tests/emu/iface_res_check
	tests/emu/iface_res_check
	LD_PRELOAD="$$($(CC) -print-file-name=libasan.so) $$($(CC) -print-file-name=libubsan.so)" ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 \
	    FREESASA_AMD_LIB=$(CURDIR)/$(ASAN_SO) python -m pytest tests/test_ingest.py tests/test_select.py tests/test_capi.py tests/test_hostfault.py tests/test_classifier.py tests/test_classifier_hostfault.py -q -m "not gpu" -p no:cacheprovider

# (-r: no built-in rules.  The reference's generated lexer.c / parser.c are compiled where they lie; make's built-in .l.c / .y.c
# rules would try to regenerate them INSIDE the reference tree whenever lexer.l / parser.y carry a later time stamp.)
oracle: $(LIBDIR)/libfreesasa_amd_seam.a
	$(MAKE) -r -C oracle all dropin
tools:
	$(MAKE) -C tools

clean:
	rm -rf $(LIBDIR) tests/emu/libsasa_emu.so tests/emu/libingest_scalar.so tests/emu/libselect_emu.so tests/emu/libgroups_emu.so tests/emu/libtraj_emu.so tests/emu/libtraj_groups_emu.so tests/emu/libtraj_pairs_emu.so tests/emu/libtraj_pair_res_emu.so tests/emu/pair_res_check tests/emu/libdcd_emu.so tests/emu/libpbc_emu.so tests/emu/libpbc_tri_emu.so tests/emu/libgroups_pbc_emu.so tests/emu/libtraj_pairs_pbc_emu.so tests/emu/libnc_emu.so tests/emu/libxtc_emu.so tests/emu/dcd_check tests/emu/cell_check tests/emu/nc_check tests/emu/xtc_check tests/emu/xtc_emu_check tests/emu/xtc_*.o tests/emu/libtrr_emu.so tests/emu/trr_check tests/emu/trr_*.o tests/emu/libstats_emu.so tests/emu/stats_check tests/emu/libvolume_emu.so tests/emu/libdots_emu.so tests/emu/dots_check tests/emu/libiface_emu.so tests/emu/iface_check tests/emu/libiface_res_emu.so tests/emu/iface_res_check tests/emu/libcontacts_emu.so tests/emu/contacts_check tests/emu/librescontacts_emu.so tests/emu/rescontacts_check tests/emu/libifsweep_emu.so tests/emu/ifsweep_check tests/emu/libocc_emu.so tests/emu/occ_check tests/emu/groups_pbc_check tests/emu/ingest_check
	$(MAKE) -C oracle clean
	$(MAKE) -C tools clean
.PHONY: all emu oracle tools clean asan asan-test
