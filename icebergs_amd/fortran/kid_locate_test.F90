!> Test driver of ignore_ij_restart through the Fortran glue: &icebergs_nml (./input.nml, with ignore_ij_restart = .true. and
!! either value of use_slow_find) -> kid_icebergs_init, which hands the two switches to the handle (kid_set_restart_locate) ->
!! kid_read_restart of <dir>/icebergs.res.nc, a file whose ine, jne are wrong on purpose: every berg's cell is searched from
!! its position (IO2:876-891).  Prints the number of bergs kept and a checksum of their cells in row order,
!! sum over rows k = 1.. of k * (ine + 1000 * jne), which tests/test_locate_fortran_gpu.py compares with the Python host's.
!!
!! The grid is the stand-alone driver's Cartesian one (driver/icebergs_driver.F90:274-286).
!! Arguments: gni gnj gridres capacity dir
program kid_locate_test
  use, intrinsic :: iso_c_binding
  use kid_hip_mod
  use kid_icebergs_glue
  implicit none
  character(len=1024) :: arg, dir
  integer :: gni, gnj, i, j, q
  real(c_double) :: gridres
  integer(c_int64_t) :: capacity, n_slots, n_alive, k, chk
  real(c_double), allocatable :: lon(:,:), lat(:,:), wet(:,:), dx(:,:), dy(:,:), area(:,:), cos_rot(:,:), sin_rot(:,:), depth(:,:)
  integer(c_int32_t), allocatable, target :: ine(:), jne(:), alive(:)
  type(kid_glue), target :: bergs
  type(kid_berg_soa) :: soa

  call get_command_argument(1, arg) ; read(arg, *) gni
  call get_command_argument(2, arg) ; read(arg, *) gnj
  call get_command_argument(3, arg) ; read(arg, *) gridres
  call get_command_argument(4, arg) ; read(arg, *) capacity
  call get_command_argument(5, dir)

  allocate(lon(0:gni+1, 0:gnj+1), lat(0:gni+1, 0:gnj+1), wet(0:gni+1, 0:gnj+1), dx(0:gni+1, 0:gnj+1), dy(0:gni+1, 0:gnj+1), &
           area(0:gni+1, 0:gnj+1), cos_rot(0:gni+1, 0:gnj+1), sin_rot(0:gni+1, 0:gnj+1), depth(0:gni+1, 0:gnj+1))
  do j = 0, gnj + 1 ; do i = 0, gni + 1
    lon(i,j) = gridres * real(i, c_double) ; lat(i,j) = gridres * real(j, c_double)
    dx(i,j) = gridres ; dy(i,j) = gridres ; area(i,j) = gridres * gridres
    wet(i,j) = 1. ; cos_rot(i,j) = 1. ; sin_rot(i,j) = 0. ; depth(i,j) = 1000.
  enddo ; enddo
  call kid_icebergs_init(bergs, gni, gnj, (/1, 1/), (/1, 1/), (/0, 0/), 0, 0, 600._c_double, 1, 0._c_double, &
                         lon(1:gni,1:gnj), lat(1:gni,1:gnj), wet, dx, dy, area(1:gni,1:gnj), cos_rot, sin_rot, &
                         ocean_depth=depth(1:gni,1:gnj), fractional_area=.false., capacity=capacity)
  call kid_check(kid_read_restart(bergs%h, trim(dir) // c_null_char), bergs%h, 'kid_read_restart')
  call kid_check(kid_num_bergs(bergs%h, n_slots, n_alive), bergs%h, 'kid_num_bergs')
  allocate(ine(max(n_slots, 1_c_int64_t)), jne(max(n_slots, 1_c_int64_t)), alive(max(n_slots, 1_c_int64_t)))
  soa%n = n_slots
  do q = 1, KID_NB_F64 ; soa%f64(q) = c_null_ptr ; enddo
  do q = 1, KID_NB_I32 ; soa%i32(q) = c_null_ptr ; enddo
  soa%id = c_null_ptr
  soa%i32(KID_BI_INE+1) = c_loc(ine) ; soa%i32(KID_BI_JNE+1) = c_loc(jne) ; soa%i32(KID_BI_ALIVE+1) = c_loc(alive)
  call kid_check(kid_download_bergs(bergs%h, soa), bergs%h, 'kid_download_bergs')
  chk = 0
  do k = 1, n_slots
    if (alive(k) == 0) error stop 'kid_locate_test: a dead row after kid_read_restart'
    chk = chk + k * (int(ine(k), c_int64_t) + 1000_c_int64_t * int(jne(k), c_int64_t))
  enddo
  write(*,'(a,i0,a,i0)') 'kid_locate_test: kept=', n_alive, ' checksum=', chk
  call kid_glue_end(bergs)
end program kid_locate_test
