!> Test driver of the debug-mode invariants in the glue (kid_glue_check_bergs): the namelist group icebergs_nml read from
!! ./input.nml, kid_icebergs_init on the stand-alone driver's Cartesian grid and a population from a case file, as
!! kid_chksum_test.F90 (the same case format and the same output), then one call of kid_icebergs_run with the ocean at rest.
!! With debug = T each of the three checksum groups of that call ends with the two lines of count_out_of_order and
!! check_for_duplicates; with debug = F none is printed.  A third argument `position` makes the program call
!! kid_glue_check_bergs itself before the run, check_position included: a population with a wrong xi stops there with the
!! reference's message.  Written and checked by tests/test_fortran_check_gpu.py.
program kid_check_test
  use, intrinsic :: iso_c_binding
  use kid_hip_mod
  use kid_icebergs_glue
  implicit none
  character(len=1024) :: fin, fout, mode
  type(kid_glue), target :: bergs
  type(iceberg) :: vals
  integer(c_int32_t) :: magic, gni, gnj, dom_x_flags, nsteps
  real(c_double) :: gridres, dt, sst0, sss0
  integer(c_int64_t) :: capacity, n, k
  integer :: u, uo_, q, s, i, j
  real(c_double), allocatable :: lon(:,:), lat(:,:), wet(:,:), dx(:,:), dy(:,:), area(:,:), cos_rot(:,:), sin_rot(:,:), depth(:,:)
  real(c_double), allocatable, target :: uo(:,:), vo(:,:), ui(:,:), vi(:,:), tauxa(:,:), tauya(:,:), ssh(:,:), sst(:,:), cn(:,:), hi(:,:), &
      sss(:,:), calving(:,:), calving_hflx(:,:)

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  mode = ' '
  if (command_argument_count() >= 3) call get_command_argument(3, mode)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
  read(u) magic
  if (magic /= 1263093767) error stop 'kid_check_test: bad magic'
  read(u) gni, gnj, dom_x_flags, nsteps
  read(u) gridres, dt, sst0, sss0
  read(u) capacity, n

  allocate(lon(0:gni+1, 0:gnj+1), lat(0:gni+1, 0:gnj+1), wet(0:gni+1, 0:gnj+1), dx(0:gni+1, 0:gnj+1), dy(0:gni+1, 0:gnj+1), &
           area(0:gni+1, 0:gnj+1), cos_rot(0:gni+1, 0:gnj+1), sin_rot(0:gni+1, 0:gnj+1), depth(0:gni+1, 0:gnj+1))
  do j = 0, gnj + 1 ; do i = 0, gni + 1
    lon(i,j) = gridres * real(i, c_double) ; lat(i,j) = gridres * real(j, c_double)
    dx(i,j) = gridres ; dy(i,j) = gridres ; area(i,j) = gridres * gridres
    wet(i,j) = 1. ; cos_rot(i,j) = 1. ; sin_rot(i,j) = 0. ; depth(i,j) = 1000.
  enddo ; enddo

  call kid_icebergs_init(bergs, gni, gnj, (/1, 1/), (/1, 1/), (/0, 0/), dom_x_flags, 0, dt, 1, 0._c_double, &
                         lon(1:gni,1:gnj), lat(1:gni,1:gnj), wet, dx, dy, area(1:gni,1:gnj), cos_rot, sin_rot, &
                         ocean_depth=depth(1:gni,1:gnj), fractional_area=.false., capacity=capacity)

  do q = 1, KID_NB_F64 ; read(u) bergs%f64(1:n, q) ; enddo
  do q = 1, KID_NB_I32 ; read(u) bergs%i32(1:n, q) ; enddo
  read(u) bergs%ids(1:n)
  close(u)
  do k = 1, n
    call row_to_node(bergs, k, vals)
    call kid_glue_add_berg(bergs, vals)
  enddo
  call kid_glue_flatten(bergs)
  if (trim(mode) == 'position') call kid_glue_check_bergs(bergs, 'kid_check_test')

  allocate(uo(gni+2, gnj+2), vo(gni+2, gnj+2), ui(gni+2, gnj+2), vi(gni+2, gnj+2), tauxa(gni, gnj), tauya(gni, gnj), &
           ssh(gni+2, gnj+2), cn(gni+2, gnj+2), hi(gni+2, gnj+2), sst(gni, gnj), sss(gni, gnj), calving(gni, gnj), calving_hflx(gni, gnj))
  uo = 0. ; vo = 0. ; ui = 0. ; vi = 0. ; tauxa = 0. ; tauya = 0. ; ssh = 0. ; cn = 0. ; hi = 0. ; sst = sst0 ; sss = sss0
  do s = 1, nsteps
    calving = 0. ; calving_hflx = 0.
    call kid_icebergs_run(bergs, 1, real(s - 1, c_double) * dt / 86400._c_double, calving, uo, vo, ui, vi, tauxa, tauya, ssh, sst, calving_hflx, cn, hi, sss=sss)
  enddo

  open(newunit=uo_, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
  write(uo_) bergs%gd ; write(uo_) bergs%par ; write(uo_) bergs%static
  close(uo_)
  write(*,'(a)') 'kid_check_test: done'
  call kid_glue_end(bergs)
end program kid_check_test
